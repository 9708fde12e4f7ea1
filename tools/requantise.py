"""Requantises the latents of an intra `.cool` image against its source by descent on D + lambda R (RdEvaluator.descend,
DESIGN.md section 4.14): every step moves latents by +-1 where the exact change of the cost is negative and the moves do not
interact.  The networks stay as they are; the new latents are range-coded by the device writer.

    python tools/requantise.py in.cool source.png out.cool --lmbda 1e-3 [--max-steps 16] [--grids 0,1,2] [--min-gain 0] [--rounds 8]

Prints bits, PSNR and cost before and after, and the moves of every step.  A candidate of the coarsest grids reaches the
whole picture and blocks every weaker one, so with all grids admitted (the default) a step is usually a single move: run with
--grids 0,1,2 first, then once more on the result without it.  --rounds 8 lets the candidates that lost a contest compete again
within the step (a few times the moves per evaluation); a coarse candidate with the best key still owns the raster."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from cool_chic_amd import DecodeBatch, EncodeBatch, RdEvaluator, writer  # noqa: E402
from cool_chic_amd.batch import FRAME_DATA_TYPES  # noqa: E402
from cool_chic_amd.bitstream.header import CoolChicHeader, FrameHeader, VideoHeader  # noqa: E402
from cool_chic_amd.quality import _planes_to_frame_data, read_source  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stream")
    ap.add_argument("source", help=".png, .ppm or .yuv of the stream's size and format")
    ap.add_argument("out")
    ap.add_argument("--lmbda", type=float, required=True)
    ap.add_argument("--max-steps", type=int, default=16)
    ap.add_argument("--min-gain", type=float, default=0.0)
    ap.add_argument("--grids", default="", help="comma-separated grids that may move (default: all; with the coarsest grids admitted a step is usually one "
                    "move, because their candidates reach the whole picture and block the rest: start with 0,1,2)")
    ap.add_argument("--rounds", type=int, default=1, help="rounds of selection per step (1 .. 64; 8 is a sensible value): losers of a round whose "
                    "winners they do not meet compete again, for more moves from the maps of one evaluation")
    a = ap.parse_args()
    with open(a.stream, "rb") as f:
        bs = f.read()
    vh, fh, ch = VideoHeader(), FrameHeader(), CoolChicHeader()
    rest = vh.read_header(bs)
    if vh.get_value("n_frames") != 1:
        raise SystemExit("an intra image is expected: one frame")
    rest = fh.read_header(rest)
    prefix = bs[:len(bs) - len(rest)]  # video and frame header: kept
    rest = ch.read_header(rest)
    n_nn, n_lat = ch.get_value("nn_n_bytes"), ch.get_value("n_bytes_latent")
    nn, payload = rest[:n_nn], rest[n_nn:n_nn + n_lat]
    if len(rest) != n_nn + n_lat:
        raise SystemExit("an intra image is expected: one cool-chic")
    bitdepth, fdt = fh.get_value("bitdepth"), FRAME_DATA_TYPES.index(fh.get_value("frame_data_type"))

    dec = DecodeBatch(0)
    dec.add(ch.raw, nn, payload, bitdepth, fdt)
    dec.run(); dec.wait()
    arch = dec.header(0)
    decoded = _planes_to_frame_data(dec.planes(0), bitdepth, FRAME_DATA_TYPES[fdt])
    source = read_source(a.source, decoded)
    latents = [torch.from_numpy(np.ascontiguousarray(dec.latent(0, g))).cuda() for g in range(arch.n_grids)]
    ptrs = [t.data_ptr() for t in latents]

    ev = RdEvaluator(0)
    ev.add(arch, nn, ptrs, source, owner=latents)
    grids = [int(g) for g in a.grids.split(",") if g != ""] or None
    reports = ev.descend(a.lmbda, a.max_steps, a.min_gain, grids, rounds=a.rounds)
    after = ev.evaluate(a.lmbda)[0]
    before = reports[0][0].before if reports else after
    for k, rep in enumerate(reports):
        st = rep[0].step
        print(f"step {k}: {st.n_candidates} candidates, {st.n_moves} moves {list(st.n_moves_grid)}, d_sse {st.d_sse}, d_bits {st.d_bits:.3f}, "
              f"d_cost {st.d_cost:.6g}" + (f", {st.n_open} still open" if a.rounds > 1 else ""))
    for label, c in (("before", before), ("after", after)):
        print(f"{label}: {c.bits:.1f} bits, PSNR {c.quality.psnr_db:.4f} dB, cost {c.cost:.9g}")

    enc = EncodeBatch(0)
    enc.add_device(arch, nn, ptrs, owner=latents)
    enc.run(); enc.wait()
    cc = enc.bytes(0)
    with open(a.out, "wb") as f:
        f.write(prefix + cc)
    # what was written decodes to the planes the last evaluation scored
    back = DecodeBatch(0)
    h2 = writer.parse_cc_header(cc)
    p, q = h2.n_bytes_header, h2.n_bytes_header + h2.nn_n_bytes
    back.add(cc[:p], cc[p:q], cc[q:], bitdepth, fdt)
    back.run(); back.wait()
    assert all(np.array_equal(x, y) for x, y in zip(back.planes(0), ev._dec.planes(0))), "the written stream does not decode to the evaluated planes"
    print(f"{a.out}: {len(prefix) + len(cc)} bytes (was {len(bs)})")
    back.close(); enc.close(); ev.close(); dec.close()


if __name__ == "__main__":
    main()
