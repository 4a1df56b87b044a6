"""Developer aid: per-loop instruction / scratch statistics of one kernel from hipcc's assembly output.
usage: asm_report.py <file.s> <mangled-name-substring> [min-VALU]
Per block with scratch or more than min-VALU (default 150) vector instructions: the counts, and among them the lane moves
(v_mov_b32_dpp), the adds that take their lane exchange as an operand (v_add_f*_dpp), the canonicalising v_max x, x, and the
multiplies / FMAs with a literal-zero source operand (a packed one counts when the operand of both halves is the literal)."""
import re, sys
from collections import Counter
txt = open(sys.argv[1]).read()
name = sys.argv[2]
min_valu = int(sys.argv[3]) if len(sys.argv) > 3 else 150
i = txt.index(name); i = txt.index('\n', txt.index(':', i)); j = txt.index('.Lfunc_end', i)
body = txt[i:j].split('\n')
# blocks: label lines
blocks = []
cur = ('entry', 0, '')
for k, l in enumerate(body):
    m = re.match(r'^(\.LBB\d+_\d+):\s*;?\s*(.*)', l)
    if m:
        blocks.append((cur[0], cur[1], k, cur[2]))
        cur = (m.group(1), k, m.group(2))
blocks.append((cur[0], cur[1], len(body), cur[2]))
print(f"{len(body)} lines, {len(blocks)} blocks")
tot = Counter()
for lab, a, b, info in blocks:
    seg = [l.strip() for l in body[a:b] if l.strip() and not l.strip().startswith((';', '.'))]
    c = Counter(x.split()[0] for x in seg)
    sc = sum(v for k, v in c.items() if k.startswith('scratch'))
    valu = sum(v for k, v in c.items() if k.startswith('v_'))
    tot.update(c)
    if sc or valu > min_valu:
        ops = [x.split(None, 1) for x in seg if x.startswith('v_')]
        src = lambda o: [t.strip() for t in re.split(r'\s+(?:op_sel|neg_|quad_perm|row_|bank_|bound_|clamp|mul:|div:)', o[1])[0].split(',')][1:] if len(o) > 1 else []
        vmaxx = sum(1 for o in ops if o[0].startswith('v_max_f') and len(src(o)) == 2 and src(o)[0] == src(o)[1])
        zmul = sum(1 for o in ops if re.match(r'v_(pk_)?(mul|fma|fmac)_f(16|32|64)', o[0]) and '0' in src(o))
        print(f"{lab:12s} lines {a:5d}-{b:5d} instrs {len(seg):4d} VALU {valu:4d} scratch {sc:3d} pk_fma {c.get('v_pk_fma_f32', 0):3d} fma64 {c.get('v_fma_f64', 0):3d} ds {sum(v for k, v in c.items() if k.startswith('ds_')):3d} "
              f"dpp_mov {c.get('v_mov_b32_dpp', 0):3d} dpp_add {sum(v for k, v in c.items() if re.match(r'v_add_f(32|64)_dpp', k)):3d} pk_add {c.get('v_pk_add_f32', 0):3d} max_xx {vmaxx:2d} zero_mul {zmul:2d}  {info[:50]}")
print('total scratch', sum(v for k, v in tot.items() if k.startswith('scratch')))
