"""Per-function comparison of two gfx950 device assembly files (hipcc --cuda-device-only -S):
which kernels' instruction streams are identical after normalising local labels, and which
kernel descriptors (.amdhsa_kernel ... .end_amdhsa_kernel: VGPR and SGPR counts, LDS and scratch
sizes).  Used to show that a source cleanup left the compiled kernels unchanged.
usage: python tools/isa_diff.py before.s after.s"""
import re
import sys


def funcs(path):
    """name -> instruction lines, name -> descriptor lines"""
    out, desc, cur, in_desc = {}, {}, None, False
    text = open(path).read()
    # (functions only: a data object's label would take the file's tail, with the unit's id, along)
    code = set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M))
    for line in text.split("\n"):
        m = re.match(r"^(_Z\S+):\s", line + " ")
        if m and m.group(1) in code:
            cur = m.group(1)
            out[cur], desc[cur] = [], []
            continue
        if cur:
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            line = re.sub(r"\.LBB\d+_\d+", "L", line)
            line = re.sub(r"\s*;.*$", "", line)  # trailing comments (basic-block numbers)
            if line.strip().startswith(";"):
                continue
            in_desc = in_desc or line.strip().startswith(".amdhsa_kernel ")
            (desc if in_desc else out)[cur].append(line)
            in_desc = in_desc and line.strip() != ".end_amdhsa_kernel"
    return out, desc


(a, da), (b, db) = funcs(sys.argv[1]), funcs(sys.argv[2])
diff = 0
for k in sorted(set(a) | set(b)):
    if k not in a or k not in b:
        print("ONLY", "before" if k in a else "after", k)
        diff += 1
        continue
    same = a[k] == b[k]
    diff += not same
    print("SAME" if same else "DIFF", len(a[k]), len(b[k]), k)
    if da[k] != db[k]:
        diff += 1
        print("DIFF-DESC", k)
        for x, y in zip(da[k], db[k]):
            if x != y:
                print("   ", x.strip(), "->", y.strip())
sys.exit(1 if diff else 0)
