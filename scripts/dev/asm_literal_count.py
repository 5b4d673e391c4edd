"""developer tool: what a kernel issues for fp64 literals and spilled scalars, region by region (usage: asm_literal_count.py file.s [kernel-name-substring]).
Reads a -DMPC_ASM_MARK=1 -S build of a solve object and counts, from one marker to the next in layout order (KKT_BEGIN#1 is the KKT phase, KKT_END#1 the glue behind it, ...):
instructions / s_mov* / of them s_mov_b32 of a 32-bit literal / v_readlane and v_writelane on the spill registers v240 .. v255 / v_accvgpr_* / s_nop; then the totals
behind the first KKT_BEGIN (the interior-point loop) with the number of distinct literal words.  The table of profiles/r20_literal_diet.md."""
import collections, re, sys
path = sys.argv[1]; key = sys.argv[2] if len(sys.argv) > 2 else "Li66511EEE"
lines = open(path).read().splitlines()
start = end = None
for i, l in enumerate(lines):
    label = l.split(";")[0].rstrip()
    if start is None and label.endswith(":") and key in label and not l.startswith("\t") and ".L" not in label: start = i
    if start is not None and ".amdhsa_kernel" in l and key in l: end = i; break
if start is None or end is None: sys.exit(f"{key}: no kernel of that name in {path}")
marker = re.compile(r";\s*([A-Z0-9_]+_(BEGIN|END))$")
SPILL = re.compile(r"v2(4\d|5[0-5]),")
def classes(t):
    op = t.split()[0]; c = ["total"]
    if op.startswith("s_mov"): c.append("s_mov")
    if op == "s_mov_b32" and re.search(r"0x[0-9a-f]+$", t): c.append("lit")
    if op == "v_readlane_b32" and SPILL.search(t): c.append("rd")
    if op == "v_writelane_b32" and SPILL.search(t): c.append("wr")
    if op.startswith("v_accvgpr"): c.append("acc")
    if op == "s_nop": c.append("nop")
    return c
cur, seen, inloop = "ENTRY", collections.Counter(), False
regions, loop, words = collections.OrderedDict(), collections.Counter(), set()
for l in lines[start:end]:
    t = l.strip(); m = marker.match(t)
    if m:
        cur = m.group(1); seen[cur] += 1; inloop = inloop or cur == "KKT_BEGIN"
        continue
    if not t or t.startswith((";", ".", "//")) or t.split(";")[0].rstrip().endswith(":"): continue
    r = regions.setdefault(f"{cur}#{seen[cur]}", collections.Counter())
    for c in classes(t):
        r[c] += 1
        if inloop: loop[c] += 1
        if inloop and c == "lit": words.add(t.split()[-1])
COLS = ("total", "s_mov", "lit", "rd", "wr", "acc", "nop")
for k, r in regions.items(): print(f"{k:22s} " + " ".join(f"{c}={r[c]:5d}" for c in COLS))
print("inside the loop:       " + " ".join(f"{c}={loop[c]:5d}" for c in COLS) + f"  distinct literal words {len(words)}")
