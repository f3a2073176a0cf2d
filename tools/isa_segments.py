#!/usr/bin/env python3
"""Instruction counts of one kernel, cut at every s_barrier and every block label, with the source functions of each stretch.

A wave alone on its SIMD takes as long as the instructions it issues, so which wave is the slow one between two barriers is a count
over the ISA, not a guess.  Dump the ISA with line tables (as for tools/isa_stats.py, plus -g1):

    hipcc --offload-arch=gfx950 -O3 -std=c++20 -S -g1 --cuda-device-only -Iinclude -Imycobotgym_amd/csrc \\
        mycobotgym_amd/csrc/mcg_hip.hip -o /tmp/mcg.s
    python tools/isa_segments.py /tmp/mcg.s step_reach_kernelILi0ELb1 [--min 20] [--barriers | --waits]

The kernel is named by any substring of its mangled name.  One line per stretch: the label it starts at, how it ends (`barrier`, a
branch, or falling into the next label), instructions in total / `_f64` / `ds_` / `s_load` / `v_accvgpr`, and the functions its `.loc`
lines fall in (function = the nearest definition above the line in that source file; counts per function).  `--barriers` prints only
the barriers, each with the last project source line before it: read the sequences of the waves side by side before a GPU run.  The counts are
static: a stretch inside a loop or behind a wave-uniform branch is listed once, whatever the path taken.

`--waits` lists instead every `s_waitcnt` with an `lgkmcnt` field that follows a scalar load not yet waited for -- the round trips a wave
alone on its SIMD pays in full unless enough instructions cover them: the barriers passed so far, the block label, the loads pending,
the instructions of cover (issued between the first pending load and the wait), the count waited for (scalar loads return out of
order: only 0 retires them) and the source line.  After each barrier, and at the end, one line sums the stretch: waits, those with
fewer than COVER (--cover N, default 20) instructions of cover, scalar loads.  Pending loads are followed in program order across
labels, so a wait behind a branch counts the loads issued above the branch.
"""
import bisect, collections, os, re, sys

argv = sys.argv[1:]
min_ins = 1
if "--min" in argv:
    k = argv.index("--min"); min_ins = int(argv[k + 1]); del argv[k:k + 2]
args = [a for a in argv if not a.startswith("--")]
if len(args) < 2:
    sys.exit(__doc__)
path, want = args[0], args[1]
cover_min = 20
if "--cover" in argv:
    k = argv.index("--cover"); cover_min = int(argv[k + 1]); del argv[k:k + 2]; args = [a for a in argv if not a.startswith("--")]; path, want = args[0], args[1]
only_barriers = "--barriers" in sys.argv
only_waits = "--waits" in sys.argv
lines = open(path).read().split("\n")

# .file N "dir" "name" (DWARF 5) or .file N "name"
files, comp_dir = {}, ""
for l in lines:
    m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m:
        f = os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
        if int(m.group(1)) == 0 and m.group(3): comp_dir = m.group(2)          # .file 0 "<compilation directory>" "<source>"
        files[int(m.group(1))] = f if os.path.isabs(f) else os.path.join(comp_dir, f)

DEF = re.compile(r'^\s*(?:template\s*<[^;{]*>\s*)?(?:MCG_DEV|__global__|__device__|static|inline)\b[^;=]*?\b([A-Za-z_]\w*)\s*\([^;]*$')
_defs = {}
def function_at(fileno, line):
    f = files.get(fileno)
    if f not in _defs:
        starts, names = [], []
        try:
            for n, l in enumerate(open(f, errors="replace"), 1):
                m = DEF.match(l)
                if m and m.group(1) not in ("if", "for", "while", "switch", "return", "static_assert", "__launch_bounds__"):
                    starts.append(n); names.append(m.group(1))
        except OSError:
            pass
        _defs[f] = (starts, names)
    starts, names = _defs[f]
    k = bisect.bisect_right(starts, line) - 1
    return names[k] if k >= 0 else os.path.basename(f or "?")

begin = next((n for n, l in enumerate(lines) if re.match(r'^_Z\w*:', l) and want in l), None)
if begin is None:
    sys.exit(f"no kernel matching {want!r} in {path}")
print(f"# {lines[begin][:-1]}")
if only_waits: print(f"# {'barriers':>8s} {'label':>12s} {'pending':>7s} {'cover':>5s} {'lgkmcnt':>7s}  source line")
else: print(f"# {'start':>12s} {'end':8s} {'instr':>6s} {'f64':>5s} {'ds':>4s} {'s_load':>6s} {'accvgpr':>7s}  functions (instructions)")

seg = dict(label="entry", ins=[], fn=collections.Counter(), src=None)
cur_fn, cur_loc, total, nbar = "?", "?", 0, 0
def flush(end):
    global seg
    ins = seg["ins"]
    if only_waits:
        if end in ("barrier", "end"):
            print(f"# stretch ending at {'barrier ' + str(nbar) if end == 'barrier' else 'the end'}: {stretch['waits']} waits after scalar loads, "
                  f"{stretch['bare']} with fewer than {cover_min} instructions of cover, {stretch['loads']} s_load, {stretch['ins']} instructions")
            stretch.update(waits=0, bare=0, loads=0, ins=0)
    elif only_barriers:
        if end == "barrier":
            print(f"barrier {nbar:3d}  after {seg['label']:>10s}  near {seg['src']}")
    elif len(ins) >= min_ins or end == "barrier":
        c = lambda p: sum(1 for i in ins if p in i)
        fns = "  ".join(f"{f} {n}" for f, n in seg["fn"].most_common(6))
        print(f"  {seg['label']:>12s} {end:8s} {len(ins):6d} {c('_f64'):5d} {sum(1 for i in ins if i.startswith('ds_')):4d} {c('s_load'):6d} {c('v_accvgpr'):7d}  {fns}")
pending, first_at = 0, 0            # scalar loads issued and not yet retired by an lgkmcnt(0); `total` when the first of them was issued
stretch = dict(waits=0, bare=0, loads=0, ins=0)
for l in lines[begin + 1:]:
    t = l.strip()
    if t.startswith((".end_amdhsa_kernel", ".section", ".Lfunc_end")):
        break
    m = re.match(r'\.loc\s+(\d+)\s+(\d+)', t)
    if m:
        f = files.get(int(m.group(1)), "?")
        if not any(d in f for d in ("/rocm", "/hip/", "/clang/", "/llvm/")):      # a runtime header's line says nothing: keep the last project line
            cur_fn = function_at(int(m.group(1)), int(m.group(2)))
            cur_loc = f"{os.path.basename(f)}:{m.group(2)} ({cur_fn})"
        continue
    m = re.match(r'^(\.LBB\w+):', l)
    if m:
        flush("label")
        seg = dict(label=m.group(1)[1:], ins=[], fn=collections.Counter(), src=None)
        continue
    if not l.startswith("\t") or not t or t.startswith((".", ";")):
        continue
    op = t.split()[0]
    seg["ins"].append(op); seg["fn"][cur_fn] += 1; total += 1; stretch["ins"] += 1
    if op.startswith(("s_load", "s_buffer_load")):
        if pending == 0: first_at = total
        pending += 1; stretch["loads"] += 1
    elif op == "s_waitcnt" and pending:
        m = re.search(r'lgkmcnt\((\d+)\)', t)
        if m:
            cover = total - first_at - 1
            stretch["waits"] += 1; stretch["bare"] += cover < cover_min
            if only_waits: print(f"  {nbar:8d} {seg['label']:>12s} {pending:7d} {cover:5d} {int(m.group(1)):7d}  {cur_loc}")
            if int(m.group(1)) == 0: pending = 0
    if op == "s_barrier":
        nbar += 1; seg["src"] = cur_loc
        flush("barrier")
        seg = dict(label="(cont.)", ins=[], fn=collections.Counter(), src=None)
flush("end")
if not only_barriers and not only_waits:
    print(f"# total {total} instructions, {nbar} s_barrier")
