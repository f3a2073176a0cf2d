#!/usr/bin/env python3
"""Per-symbol comparison of two device-assembly files: did an edit leave the instruction streams as they were?

    python tools/isa_identity.py parent/mcg_hip.s new/mcg_hip.s

Each .s comes from the command in tools/isa_stats.py's docstring, once in a checkout of each commit.  Per symbol: SAME or DIFF, the
instruction counts (first file / second file), and for a kernel .vgpr_count / .sgpr_count / .private_segment_fixed_size /
.group_segment_fixed_size of its metadata entry (one figure where both files agree, "a -> b" where they do not: that is a DIFF too).
A symbol's stream is what lies between its label and its .Lfunc_end, with comments, directives and label definitions dropped and
.LBB* operands renamed by order of first appearance, so that a block renumbered by an unrelated function compares equal.  The streams
are compared as text; the tool knows no instruction.  Exit status 1 if any symbol differs or exists in one file only.

    python tools/isa_identity.py parent/mcg_sac.s new/mcg_sac.s 12sac_q_kernel=8q_kernel

Further arguments old=new rename a kernel that an edit merged with another: every occurrence of `old` in the first file's text (the
mangled name's length prefix included) reads `new` before the comparison.
"""
import re, sys

FIGURES = ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')

def streams(text):
    out, name, cur, labels = {}, None, None, None
    for line in text.split('\n'):
        m = re.match(r'^([A-Za-z_$][\w$.]*):', line)
        if name is None:
            if m and not m.group(1).startswith('.L'): name, cur, labels = m.group(1), [], {}
            continue
        if line.startswith('.Lfunc_end'):
            out[name] = cur; name = None
            continue
        s = line.split(';', 1)[0].strip()
        if not s or s.startswith('.') or re.match(r'^[\w$.]+:$', s): continue
        cur.append(re.sub(r'\.LBB\d+_\d+', lambda b: labels.setdefault(b.group(0), '.LBB#%d' % len(labels)), s))
    return out

def figures(text):
    out = {}
    for entry in re.split(r'\n  - ', text[text.find('amdhsa.kernels:'):])[1:]:
        name = re.search(r'^    \.name:\s*(\S+)', entry, re.M)            # (the kernel's own keys: four spaces; its arguments' lie deeper)
        if name: out[name.group(1)] = tuple((re.search(r'^ {0,4}%s:\s*(\d+)' % re.escape(f), entry, re.M) or [None, '?'])[1] for f in FIGURES)
    return out

def main(a_path, b_path, *renames):
    a, b = open(a_path).read(), open(b_path).read()
    for old, new in (r.split('=', 1) for r in renames): a = a.replace(old, new)
    sa, sb, fa, fb = streams(a), streams(b), figures(a), figures(b)
    same = diff = 0
    for sym in sorted(set(sa) | set(sb)):
        if sym not in sa or sym not in sb:
            print(f"DIFF  {len(sa.get(sym, [])):6d}  {len(sb.get(sym, [])):6d}  {sym}  (in one file only)"); diff += 1
            continue
        ok = sa[sym] == sb[sym] and fa.get(sym) == fb.get(sym)
        fig = ''
        if sym in fa or sym in fb:
            x, y = fa.get(sym, ('?',) * 4), fb.get(sym, ('?',) * 4)
            fig = '  vgpr/sgpr/private/group ' + '/'.join(p if p == q else f"{p} -> {q}" for p, q in zip(x, y))
        print(f"{'SAME' if ok else 'DIFF'}  {len(sa[sym]):6d}  {len(sb[sym]):6d}  {sym}{fig}")
        same += ok; diff += not ok
    print(f"# {same} SAME, {diff} DIFF")
    return 1 if diff else 0

if __name__ == '__main__':
    if len(sys.argv) < 3 or not all('=' in r for r in sys.argv[3:]): sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
