"""Developer aid: per-kernel comparison of two gfx950 assembly listings of the library, to show that a host-side or file-layout change
left the device code of a kernel alone.  Produce each listing with the Makefile's flags plus `-S --cuda-device-only`
(hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-variable -S --cuda-device-only -o a.s mpcqp_kernels.hip).
A kernel is its text from the symbol's label to its .Lfunc_end, without comments, .loc / .file / .cfi / .p2align lines and the
function index in local labels (.LBB<n>_<m> -> .LBB_<m>): position in the module does not leak into a kernel's code.
usage: python tools/isa_compare.py a.s b.s [renames.txt]     prints same / DIFF / ONLY per kernel symbol, and under a DIFF line the
mnemonics whose counts differ; exit status 1 when any differs
renames.txt: lines `old_symbol new_symbol` for kernels that were renamed between the listings.  a[old] is compared with b[new] after
every occurrence of the old symbol in a[old]'s text (its .amdhsa_kernel and .section lines, labels) is replaced by the new one."""
import re, sys
from collections import Counter


def kernels(path):
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", open(path).read(), re.S | re.M):
        lines = []
        for l in m.group(2).split("\n"):
            s = l.split(";")[0].rstrip()
            if s.strip() and not s.strip().startswith((".loc", ".file", ".cfi", ".p2align")):
                lines.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s))
        out[m.group(1)] = lines
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
print(f"{len(a)} / {len(b)} kernels")
was = {}
for old, new in (l.split() for l in (open(sys.argv[3]) if len(sys.argv) > 3 else []) if l.strip()):
    if old in a and new not in a:   # (a pair that does not apply is left to show as ONLY)
        a[new] = [l.replace(old, new) for l in a.pop(old)]
        was[new] = " <- " + old
bad = 0
for k in sorted(set(a) | set(b)):
    if k not in a or k not in b:
        print("ONLY", "a" if k in a else "b", k)
    else:
        print("same" if a[k] == b[k] else "DIFF", len(a[k]), len(b[k]), k + was.get(k, ""))
        if a[k] != b[k]:   # per-mnemonic counts that differ (instructions only: neither labels nor directives)
            ca, cb = (Counter(l.split()[0] for l in t if l[0].isspace() and not l.strip().startswith(".")) for t in (a[k], b[k]))
            print("    ", ", ".join(f"{m} {ca[m]} -> {cb[m]}" for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m]) or "same count of every mnemonic")
    bad += k not in a or k not in b or a[k] != b[k]
sys.exit(1 if bad else 0)
