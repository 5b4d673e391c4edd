"""developer tool: per KERNEL of the object files of a build (kernel_device_hash.py <dir with *.o>), the sha256 of its gfx950 disassembly without addresses and without the
branch-target comments, so that a kernel keeps its hash when a neighbour in the same object changes size (obj_device_hash.sh hashes whole objects).  Two builds whose
lines are equal run the same instructions in those kernels; registers and scratch are in the notes obj_device_hash.sh hashes and kernel_resources.sh prints."""
import glob, hashlib, os, re, shutil, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"
for o in sorted(glob.glob(os.path.join(sys.argv[1], "*.o"))):
    t = tempfile.mkdtemp()
    shutil.copy(o, os.path.join(t, "o.o"))
    subprocess.run([LLVM + "/llvm-objdump", "--offloading", "o.o"], cwd=t, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for f in glob.glob(os.path.join(t, "o.o.*gfx950")):
        dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", f], capture_output=True, text=True).stdout
        name, h, n, pc = None, None, 0, 0
        def flush():
            if name: print(f"{os.path.basename(o)} {h.hexdigest()[:16]} ({n} instructions) {name}")
        for l in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", l)
            if m:
                flush(); name, h, n = m.group(1), hashlib.sha256(), 0
            elif name and l.startswith(("\t", " ")) and l.strip():
                ins = l.split("//")[0].strip()
                if ins.startswith("s_getpc_b64"): pc = 2      # the two adds behind it form the pc-relative address of a callee or a table: it moves with the object's layout
                elif pc > 0 and ins.startswith(("s_add_u32", "s_addc_u32")): ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins); pc -= 1
                h.update((ins + "\n").encode()); n += 1
        flush()
    shutil.rmtree(t)
