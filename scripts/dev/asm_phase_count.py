"""Static instruction counts between the `; XXX_BEGIN` / `; XXX_END` markers of a -DMPC_ASM_MARK=1 -S build of a solve object
(usage: asm_phase_count.py file.s kernel-name-substring).  Counts by class: VALU (v_*), of which DPP, division helpers, transcendental; SALU; LDS; readlane / writelane;
waitcnt / nop.  After the phases: the GAPS, the instructions between one phase's END marker and the next BEGIN marker in program order (the solve loop's
wave-uniform code), and what follows the last marker up to the end of the kernel (loop back edge + epilogue).  Loops and branches are counted once (static)."""
import re, sys, collections
path, key = sys.argv[1], sys.argv[2]
lines = open(path).read().splitlines()
# the function body: from the label line "<mangled>:" (which may carry a trailing "; @<mangled>" comment) to its .amdhsa_kernel
start = end = None
for i, l in enumerate(lines):
    label = l.split(";")[0].rstrip()
    if start is None and label.endswith(":") and key in label and not l.startswith("\t") and ".L" not in label: start = i
    if start is not None and ".amdhsa_kernel" in l and key in l: end = i; break
if start is None or end is None: sys.exit(f"{key}: no kernel of that name in {path}")
body = lines[start:end]
print(f"{key}: lines {start}..{end}")
stack = {}; res = collections.OrderedDict()
gaps = []; gap = None; last = "KERNEL_ENTRY"
def cls(op):
    c = []
    if op.startswith("v_"):
        c.append("valu")
        if "readlane" in op or "writelane" in op or "readfirstlane" in op: c.append("lane_x")
        if op.startswith(("v_div_", "v_rcp", "v_rsq", "v_sqrt", "v_log", "v_exp", "v_ldexp", "v_frexp")): c.append("div/trans")
        if op.startswith("v_cmp"): c.append("cmp")
        if op.startswith("v_cndmask"): c.append("cndmask")
        if op.startswith(("v_accvgpr", "v_mov")): c.append("mov")
        if op.startswith("v_accvgpr"): c.append("agpr")
    elif op.startswith("s_"):
        if op.startswith(("s_waitcnt", "s_nop", "s_barrier")): c.append("wait/nop")
        elif op.startswith(("s_cbranch", "s_branch")): c.append("branch")
        else: c.append("salu")
    elif op.startswith("ds_"): c.append("lds")
    elif op.startswith(("global_", "buffer_", "scratch_", "flat_")): c.append("vmem")
    else: c.append("other")
    return c
def show(name, c): print(f"{name:44s} " + "  ".join(f"{k}={v}" for k, v in sorted(c.items(), key=lambda kv: -kv[1])))
marker = re.compile(r";\s*([A-Z0-9_]+)_(BEGIN|END)$")
paired = {m.group(1) for m in (marker.match(l.strip()) for l in body) if m and m.group(2) == "END"}      # a BEGIN without an END anywhere (BWD_SETUP) is a point: it only cuts a gap
for l in body:
    t = l.strip()
    m = marker.match(t)
    if m:
        name, what = m.groups()
        if name not in paired:
            if gap is not None and not stack: gaps.append((f"{last} -> {name}_BEGIN", gap)); gap = collections.Counter(); last = f"{name}_BEGIN"
        elif what == "BEGIN":
            stack[name] = collections.Counter()
            if gap is not None and not [n for n in stack if n != name]: gaps.append((f"{last} -> {name}_BEGIN", gap))
            gap = None
        else:
            c = stack.pop(name, None)
            if c is not None: res.setdefault(name, []).append(c)
            if not stack: gap = collections.Counter(); last = f"{name}_END"
        continue
    if not t or t.startswith((";", ".", "//")) or t.split(";")[0].rstrip().endswith(":"): continue
    op = t.split()[0]
    dpp = "row_" in t or "quad_perm" in t or "wave_" in t
    for c in list(stack.values()) + ([gap] if gap is not None and not stack else []):
        c["total"] += 1
        for k in cls(op): c[k] += 1
        if dpp: c["dpp"] += 1
if gap is not None: gaps.append((f"{last} -> end of the kernel", gap))
print("-- phases")
for name, cs in res.items():
    for c in cs: show(name, c)
print("-- gaps (program order)")
for name, c in gaps: show(name, c)
