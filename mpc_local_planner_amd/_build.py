"""Build-if-stale for the native code (the HIP library, its instrumented copies, the tests' host harnesses): the dependencies come from the compiler, not from a list.

Every compile step runs with -MMD -MF; after a successful build the depfiles are folded into a stamp next to the output (<output>.stamp): the commands (without
the compiler's own path) and the dependencies, both relative to the tree.  An output is stale when it or its stamp is missing, the commands differ, or a recorded
dependency is missing or newer than the output.  Nothing in the stamp is absolute, so a tree copied elsewhere with its outputs (and their mtimes) is not stale there.
Plain Python: imports neither torch nor the library.
"""
import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SOURCE = (".c", ".cc", ".cpp", ".hip")


def _recorded(commands, root):
    return [[a.replace(root + os.sep, "") for a in cmd[1:]] for cmd in commands]


def _dependencies(depfile, cwd, root):
    """the prerequisites of a Makefile-syntax depfile, relative to `root` where they lie inside it"""
    deps = set()
    for rule in open(depfile).read().replace("\\\n", " ").splitlines():
        for d in re.findall(r"(?:\\ |\S)+", rule.partition(": ")[2]):
            path = os.path.normpath(os.path.join(cwd, d.replace("\\ ", " ").replace("$$", "$")))
            deps.add(os.path.relpath(path, root) if path.startswith(root + os.sep) else path)
    return deps


def stale(out, commands, root=ROOT) -> bool:
    try:
        with open(out + ".stamp") as f:
            stamp = json.load(f)
        t = os.path.getmtime(out)
    except (OSError, ValueError):
        return True
    if stamp["commands"] != _recorded(commands, root):
        return True
    deps = [os.path.join(root, d) for d in stamp["deps"]]
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in deps)


def build(out, commands, cwd, root=ROOT, force=False, verbose=False) -> bool:
    """Runs `commands` (argv lists; the last one writes `out`, the ones before it are independent of each other and run in parallel) when `out` is stale.
    True when it compiled."""
    commands = [list(c) for c in commands]
    if not force and not stale(out, commands, root):
        return False
    if os.path.exists(out + ".stamp"):
        os.remove(out + ".stamp")
    depfiles = []

    def run(cmd):
        target = cmd[cmd.index("-o") + 1]
        os.makedirs(os.path.dirname(target), exist_ok=True)
        if any(a.endswith(_SOURCE) for a in cmd):      # a compile step
            depfiles.append(target + ".d")
            cmd = cmd + ["-MMD", "-MF", target + ".d"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, cwd=cwd)
    with ThreadPoolExecutor(max_workers=min(len(commands), os.cpu_count() or 2)) as pool:
        list(pool.map(run, commands[:-1]))
    run(commands[-1])
    deps = set()
    for d in depfiles:
        deps |= _dependencies(d, cwd, root)
        os.remove(d)
    with open(out + ".stamp", "w") as f:
        json.dump({"commands": _recorded(commands, root), "deps": sorted(deps)}, f, indent=0)
    return True
