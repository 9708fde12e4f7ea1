#!/usr/bin/env python3
"""Counts the producers' late path in the ISA of the pipelined entropy kernel ("The late path, trimmed" and "The
output tail, from registers"), so that the tables there can be continued the same way.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -S --cuda-device-only \\
          cool_chic_amd/csrc/ccd_entropy_pipe.hip -o pipe.s
    python tools/count_late_path.py pipe.s [kernel name substring = the production instantiation]

The rule.  In the kernel, every `s_setprio 1` opens the late path of one producer instantiation (8-, 4-, 2-pixel tasks: told apart
by their multiply-adds, 71-84 / 48-63 / 25-42).  The path of a full task of narrow pixels runs from there, fall-through, to the
`s_cbranch_scc1` that jumps to the block holding the ready bit's `ds_or_b32` (taken: no pixel of the task needs the wide window),
and from that block's label to the `ds_or_b32`.  Counted: every instruction on it, both ends and the branches included, `s_nop n`
as one; not counted: labels, directives, comments.  Also printed: the `s_nop`, `s_waitcnt`, LDS reads and spill-lane moves on it."""
import re
import sys

PROD = "entropy_pipe_kernelILi5ELb0ELb0ENS_8ShapeFixILi20ELi3ELi14EEEEE"


def is_instr(line):
    t = line.strip()
    return line.startswith("\t") and t and not t.startswith((";", "."))


def main():
    path, want = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else PROD)
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and want in l.split(":")[0] and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    k = lines[start:end]
    for s in [i for i, l in enumerate(k) if "s_setprio 1" in l]:
        o = next(i for i in range(s, len(k)) if "ds_or_b32" in k[i])
        lab_i = max(i for i in range(s, o) if re.match(r"\.LBB\d+_\d+:", k[i]))
        lab = k[lab_i].split(":")[0]
        br = next(i for i in range(s, lab_i) if re.match(r"\s*s_cbranch_scc1\s+%s\b" % re.escape(lab), k[i]))
        ins = [l.strip() for l in k[s:br + 1] + k[lab_i:o + 1] if is_instr(l)]
        n = lambda pat: sum(1 for l in ins if re.match(pat, l))
        print(f"{len(ins):4d} instructions   v_mad_i64_i32 {n('v_mad_i64_i32'):3d}   s_nop {n('s_nop'):2d}   s_waitcnt {n('s_waitcnt'):2d}   "
              f"ds_read {n('ds_read'):2d}   ds_write {n('ds_write'):2d}   v_readlane/v_writelane {n('v_(read|write)lane'):2d}   scratch {n('scratch_'):d}")


if __name__ == "__main__":
    main()
