#!/usr/bin/env python3
"""Compares the kernels of two assembly files of the same source, e.g. the pipelined entropy kernel before and after a change
that must not alter the compiled code ("Reading the producers").

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -S --cuda-device-only \\
          -Rpass-analysis=kernel-resource-usage cool_chic_amd/csrc/ccd_entropy_pipe.hip -o a.s 2> a.log
    python tools/isa_compare.py a.s b.s [a.log b.log]

For every kernel symbol present in both files: `identical`, or the first instruction that differs.  Comments, directives and blank
lines are dropped and labels renumbered in order of appearance first.  With the two -Rpass-analysis logs, the resource lines of
every kernel are printed side by side."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        if name is None:
            m = re.match(r"(_Z\w+):", line)
            name, body = (m.group(1), []) if m else (None, [])
        elif line.startswith(".Lfunc_end"):
            out[name], name = body, None
        else:
            t = line.split(";")[0].strip()
            if t and not (t.startswith(".") and not t.endswith(":")):
                body.append(t)
    for body in out.values():  # label numbering: by first appearance
        ids = {}
        for i, t in enumerate(body):
            body[i] = re.sub(r"\.L\w+", lambda m: ids.setdefault(m.group(0), ".L%d" % len(ids)), t)
    return out


def resources(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1).startswith("Function Name:"):
            name = m.group(1).split(":", 1)[1].strip()
            out[name] = []
        elif name and re.match(r"(TotalSGPRs|VGPRs|ScratchSize|SGPRs Spill|VGPRs Spill|Occupancy)\b", m.group(1)):
            out[name].append(m.group(1))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    res = [resources(p) for p in sys.argv[3:5]]
    for k in [k for k in a if k in b]:
        d = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), None)
        if d is None and len(a[k]) == len(b[k]):
            print(f"{k}: identical ({len(a[k])} lines)")
        else:
            d = min(len(a[k]), len(b[k])) if d is None else d
            print(f"{k}: DIFFERENT at line {d} of {len(a[k])} / {len(b[k])}: {(a[k] + ['<end>'])[d]!r} / {(b[k] + ['<end>'])[d]!r}")
        if len(res) == 2:
            print("    a: " + "; ".join(res[0].get(k, [])) + "\n    b: " + "; ".join(res[1].get(k, [])))


if __name__ == "__main__":
    main()
