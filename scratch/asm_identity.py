"""Compares two device-assembly files (hipcc -S --cuda-device-only) function by function: comments, labels and directives are
stripped and the function index is taken out of basic-block label names (the method of profiles/twin_base/asm_identity.txt).
usage: python scratch/asm_identity.py parent.s new.s"""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m:
            if name:
                out[name] = body
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") and not s.startswith(".LBB") or s.endswith(":"):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    if name:
        out[name] = body
    return out


a, b = functions(sys.argv[1]), functions(sys.argv[2])
same = [n for n in a if n in b and a[n] == b[n]]
diff = [n for n in a if n in b and a[n] != b[n]]
print("%d functions at the parent, %d in this build; %d identical, %d differ, %d only at the parent, %d only in this build" %
      (len(a), len(b), len(same), len(diff), len(set(a) - set(b)), len(set(b) - set(a))))
for n in diff:
    print("  differs  %-100s instructions %d -> %d" % (n, len(a[n]), len(b[n])))
for n in sorted(set(a) - set(b)):
    print("  only at the parent  %s (%d)" % (n, len(a[n])))
for n in sorted(set(b) - set(a)):
    print("  only in this build  %s (%d)" % (n, len(b[n])))
