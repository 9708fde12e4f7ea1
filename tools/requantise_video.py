"""Requantises the latents of every frame of a `.cool` video against its source by descent on D + lambda R (DESIGN.md sections
4.14 and 4.15).  The frames are walked in coding order: I frames go through RdEvaluator.descend as in tools/requantise.py, P / B
frames through InterRdEvaluator.descend with the planes of the already REQUANTISED frames as their references.  The networks and
every header stay as they are; the new latents of each cool-chic are range-coded by the device writer.
With --follow an I frame does not finish before its dependents start: it descends TOGETHER with the residues of the
P / B frames that predict from it directly and whose other reference, if any, is already requantised (GopDescent: the steps are
priced by own + dependent deltas and their claims follow the flows).  Those frames then go through their own descent as usual.

    python tools/requantise_video.py in.cool source.yuv out.cool --lmbda 1e-3 [--max-steps 16] [--grids 0,1,2] [--min-gain 0] [--joint]
                                     [--follow]

Prints bits, PSNR and cost of every frame before and after ("before": the stream's latents against the references as they are now,
requantised), writes the stream, decodes it back with decode_video and asserts that every frame's planes are those the last
evaluation scored."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from cool_chic_amd import DecodeBatch, EncodeBatch, GopDescent, InterRdEvaluator, RdEvaluator  # noqa: E402
from cool_chic_amd.bitstream.decode import _split_frame, decode_video  # noqa: E402
from cool_chic_amd.bitstream.header import VideoHeader  # noqa: E402
from cool_chic_amd.quality import read_source  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stream")
    ap.add_argument("source", help="planar .yuv (or .png / .ppm for one frame) of the stream's size and format; frame d = display index d")
    ap.add_argument("out")
    ap.add_argument("--lmbda", type=float, required=True)
    ap.add_argument("--max-steps", type=int, default=16, help="per frame")
    ap.add_argument("--min-gain", type=float, default=0.0)
    ap.add_argument("--grids", default="", help="comma-separated grids that may move, in every cool-chic (default: all; see tools/requantise.py)")
    ap.add_argument("--rounds", type=int, default=1, help="rounds of selection per step (1 .. 64; 8 is a sensible value; see tools/requantise.py)")
    ap.add_argument("--joint", action="store_true", help="P / B frames: every step moves both cool-chics (InterRdEvaluator.descend(joint=True))")
    ap.add_argument("--follow", action="store_true",
                    help="an I frame and the residues of its direct dependents move in one descent whose claims follow the flows (GopDescent)")
    a = ap.parse_args()
    grids = [int(g) for g in a.grids.split(",") if g != ""] or None
    with open(a.stream, "rb") as f:
        bs = f.read()
    vh = VideoHeader()
    rest = vh.read_header(bs)
    n_frames = vh.get_value("n_frames")
    structure = vh.get_coding_structure()
    parsed = []
    for _ in range(n_frames):
        fh, ccs, rest = _split_frame(rest)
        parsed.append((fh, ccs))
    display = [int(structure[k]["display_order"]) for k in range(n_frames)]
    coding_of = {d: k for k, d in enumerate(display)}
    original = decode_video(a.stream)  # {display index: FrameData}: sizes and formats of the sources
    sources = [read_source(a.source, original[str(display[k])], frame_index=display[k]) for k in range(n_frames)]

    # the latents of every cool-chic, entropy-decoded once; they stay on the device and are moved in place
    dec = DecodeBatch(0)
    slots = [[dec.add(ch.raw, nn, lat, 0, 0) for ch, nn, lat in ccs] for _, ccs in parsed]
    dec.run(); dec.wait()
    cool_chics = []  # per frame: [(arch, nn, [device tensors])]
    for k, (_, ccs) in enumerate(parsed):
        row = []
        for s, (_, nn, _) in zip(slots[k], ccs):
            arch = dec.header(s)
            row.append((arch, nn, [torch.from_numpy(np.ascontiguousarray(dec.latent(s, g))).cuda() for g in range(arch.n_grids)]))
        cool_chics.append(row)
    dec.close()

    def references(k):
        n_refs = "IPB".index(parsed[k][0].get_value("frame_type"))
        return [coding_of[int(r)] for r in structure[k]["index_references"]][:n_refs]

    done = {}  # coding index -> the device planes of the requantised frame, as its last evaluation scored them
    for k, (fh, _) in enumerate(parsed):
        frame_type = fh.get_value("frame_type")
        ptrs = [[t.data_ptr() for t in lat] for _, _, lat in cool_chics[k]]
        if frame_type == "I":
            ev = RdEvaluator(0)
            arch, nn, lat = cool_chics[k][0]
            ev.add(arch, nn, ptrs[0], sources[k], owner=lat)
            # --follow: the frames that predict from this one directly and have no other reference still to come
            group = [j for j in range(k + 1, n_frames) if a.follow and k in references(j) and all(r == k or r in done for r in references(j))]
            if group:
                inter = InterRdEvaluator(0)
                gop = GopDescent(ev, inter)
                for j in group:
                    (ra, rn, rl), (ma, mn, ml) = cool_chics[j]
                    fj = parsed[j][0]
                    inter.add(fj.get_value("frame_type"), (ra, rn, [t.data_ptr() for t in rl]), (ma, mn, [t.data_ptr() for t in ml]),
                              [gop.reference_planes(0) if r == k else done[r] for r in references(j)], fj.get_value("global_flow"),
                              fj.get_value("warp_filter_size"), sources[j], owner=(rl, ml))
                for f, j in enumerate(group):
                    for which, r in enumerate(references(j)):
                        if r == k:
                            gop.follow(0, f, which)
                steps = gop.descend(a.lmbda, a.max_steps, a.min_gain, grids, rounds=a.rounds)
                after = ev.evaluate(a.lmbda)[0]
                gop.close(); inter.close()
                moves = [(f"{r.slots[0].step.n_moves} + {sum(s.step.n_moves for s in r.slots[1:])}",
                          f" intra + residues of {', '.join(str(display[j]) for j in group)}") for r in steps]
                before = steps[0].intra[0] if steps else after
            else:
                reports = ev.descend(a.lmbda, a.max_steps, a.min_gain, grids, rounds=a.rounds)
                after = ev.evaluate(a.lmbda)[0]
                moves = [(r[0].step.n_moves, "") for r in reports]
                before = reports[0][0].before if reports else after
            done[k] = [p.clone() for p in ev.planes(0)]
        else:
            refs = references(k)
            ev = InterRdEvaluator(0)
            (ra, rn, rl), (ma, mn, ml) = cool_chics[k]
            ev.add(frame_type, (ra, rn, ptrs[0]), (ma, mn, ptrs[1]), [done[r] for r in refs], fh.get_value("global_flow"),
                   fh.get_value("warp_filter_size"), sources[k], owner=(rl, ml))
            reports = ev.descend(a.lmbda, a.max_steps, a.min_gain, grids, rounds=a.rounds, joint=a.joint)
            after = ev.evaluate(a.lmbda)[0]
            done[k] = [p.clone() for p in ev.planes(0)]
            if a.joint:
                moves = [(f"{r[0].steps[0].n_moves} + {r[0].steps[1].n_moves}", " residue + motion") for r in reports]
            else:
                moves = [(r[0].step.n_moves, " " + r[0].role) for r in reports]
            before = reports[0][0].before if reports else after
        print(f"frame {display[k]} ({frame_type}): steps " + ", ".join(f"{n}{role}" for n, role in moves))
        for label, c in (("before", before), ("after", after)):
            print(f"  {label}: {c.bits:.1f} bits, PSNR {c.quality.psnr_db:.4f} dB, cost {c.cost:.9g}")
        ev.close()

    # every cool-chic through the device writer, the headers of the stream kept
    enc = EncodeBatch(0)
    for row in cool_chics:
        for arch, nn, lat in row:
            enc.add_device(arch, nn, [t.data_ptr() for t in lat], owner=lat)
    enc.run(); enc.wait()
    out, s = [vh.raw], 0
    for (fh, _), row in zip(parsed, cool_chics):
        out.append(fh.raw)
        for _ in row:
            out.append(enc.bytes(s))
            s += 1
    enc.close()
    data = b"".join(out)
    with open(a.out, "wb") as f:
        f.write(data)
    # what was written decodes to the planes the last evaluations scored
    back = decode_video(a.out)
    for k in range(n_frames):
        fd = back[str(display[k])]
        want = [p.cpu().numpy() for p in done[k]]
        assert all(np.array_equal(x, y) for x, y in zip(fd.integer_planes(), want)), \
            f"frame {display[k]} of the written stream does not decode to the evaluated planes"
    print(f"{a.out}: {len(data)} bytes (was {len(bs)})")


if __name__ == "__main__":
    main()
