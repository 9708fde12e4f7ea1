"""Searches the quantisation steps of the networks of an intra `.cool` image against its source (NetworkQuantiser, DESIGN.md
section 4.18): float parameters + the stream's latents + a source in, a `.cool` file out.

    python tools/quantise_networks.py in.cool source.png out.cool --lmbda 1e-3 [--params floats.npz] [--sweeps N]
                                      [--fast-path-only] [--refine-arm N | --refine-rate N] [--descend STEPS]

The architecture and the latents are the input stream's.  --params: an .npz whose array `values` holds the float32 parameters
in stream order (writer.network_layout); without it the stream's own networks are dequantised and searched again.
--refine-arm runs at most N steps of the +-1 descent over the ARM's integers on the searched network (nnrefine.ArmRefiner,
DESIGN.md section 4.20: rate only, the planes stay); --refine-rate the same descent over both rate networks, the ARM's and the
IFCE's integers (nnrefine.RateRefiner, section 4.21).  --descend
runs RdEvaluator.descend (8 rounds per step) on the result for at most STEPS steps.  Prints the chosen steps, payload bytes,
bits, PSNR and cost beside the input stream's own, writes the stream and checks that it decodes to the planes that were scored."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from cool_chic_amd import DecodeBatch, EncodeBatch, RdEvaluator, writer  # noqa: E402
from cool_chic_amd.batch import FRAME_DATA_TYPES  # noqa: E402
from cool_chic_amd.bitstream.header import CoolChicHeader, FrameHeader, VideoHeader  # noqa: E402
from cool_chic_amd.nnquant import NetworkQuantiser  # noqa: E402
from cool_chic_amd.nnrefine import ArmRefiner, RateRefiner  # noqa: E402
from cool_chic_amd.quality import _planes_to_frame_data, read_source  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stream")
    ap.add_argument("source", help=".png, .ppm or .yuv of the stream's size and format")
    ap.add_argument("out")
    ap.add_argument("--lmbda", type=float, required=True)
    ap.add_argument("--params", default="", help=".npz with `values`: float32 parameters in stream order (default: the stream's own, dequantised)")
    ap.add_argument("--sweeps", type=int, default=1)
    ap.add_argument("--fast-path-only", action="store_true", help="only networks whose ARM fits the pipelined entropy kernel")
    ap.add_argument("--refine-arm", type=int, default=0, metavar="N", help="ArmRefiner.refine on the searched network, at most N steps")
    ap.add_argument("--refine-rate", type=int, default=0, metavar="N", help="RateRefiner.refine (ARM and IFCE) on the searched network, at most N steps")
    ap.add_argument("--refine-batch", type=int, default=1, help="moves tried together per step of --refine-arm / --refine-rate")
    ap.add_argument("--descend", type=int, default=0, metavar="STEPS", help="RdEvaluator.descend on the result, at most STEPS steps")
    a = ap.parse_args()
    if a.refine_arm > 0 and a.refine_rate > 0:
        raise SystemExit("--refine-arm or --refine-rate, not both")
    n_refine = max(a.refine_arm, a.refine_rate)
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
    if a.params:
        with np.load(a.params) as z:
            floats = np.asarray(z["values"], dtype=np.float32)
    else:
        floats = writer.dequantise_network(arch, writer.network_values(arch, nn))

    with RdEvaluator(0) as ev:
        ev.add(arch, nn, ptrs, source, owner=latents)
        own = ev.evaluate(a.lmbda)[0]
    res = NetworkQuantiser(0).search(arch, floats, ptrs, source, a.lmbda, sweeps=a.sweeps, fast_path_only=a.fast_path_only, owner=latents)
    for t, how in zip(res.tables, res.pricing):
        print(f"sweep {t.sweep} {t.module}: {len(t.cells)} candidates, {sum(c.feasible for c in t.cells)} feasible, {how.chunk} per launch, {how.seconds:.3f} s"
              + ("" if t.chosen is None else f", chose (2^{t.cells[t.chosen].q_w}, 2^{t.cells[t.chosen].q_b}) cost {t.cells[t.chosen].cost:.9g}"))
    rows = [("stream", own, len(nn), list(arch.nn_q_step_log2)), ("searched", res.candidate, len(res.bytes_nn), list(res.header.nn_q_step_log2))]
    searched = res.candidate
    if n_refine > 0:
        refiner = RateRefiner(0) if a.refine_rate > 0 else ArmRefiner(0)
        fine = refiner.refine(res.header, res.values, ptrs, n_refine, batch=a.refine_batch, owner=latents)
        for k, step in enumerate(fine.log):
            print(f"refine {k}: {[(m.index, m.sign) for m in step.moves]}, objective {step.objective:.3f} (predicted {step.predicted:.3f}), "
                  f"{step.n_bytes_nn} bytes of networks, {len(step.rejected)} larger batches rejected")
        print(f"refine: {len(fine.log)} steps ({fine.stopped}), objective {fine.start_objective:.3f} -> "
              f"{fine.log[-1].objective if fine.log else fine.start_objective:.3f} bits")
        res = res._replace(header=fine.header, bytes_nn=fine.bytes_nn, values=fine.values)
    with RdEvaluator(0) as ev, EncodeBatch(0) as enc, DecodeBatch(0) as back:
        ev.add(res.header, res.bytes_nn, ptrs, source, owner=latents)
        after = ev.evaluate(a.lmbda)[0]
        if n_refine > 0:  # the ARM's and the IFCE's integers move the rate alone
            assert after.mse == searched.mse and after.cost <= searched.cost
            rows.append(("refined", after, len(res.bytes_nn), list(res.header.nn_q_step_log2)))
        else:
            assert (after.mse, after.bits, after.cost) == (searched.mse, searched.bits, searched.cost)
        if a.descend > 0:
            for k, rep in enumerate(ev.descend(a.lmbda, a.descend, rounds=8)):
                print(f"step {k}: {rep[0].step.n_moves} moves, d_cost {rep[0].step.d_cost:.6g}")
            rows.append(("descended", ev.evaluate(a.lmbda)[0], len(res.bytes_nn), list(res.header.nn_q_step_log2)))
        for label, c, n, q in rows:
            print(f"{label}: steps 2^{q}, {n} bytes of networks, {c.bits:.1f} bits, PSNR {c.quality.psnr_db:.4f} dB, cost {c.cost:.9g}")

        enc.add_device(res.header, res.bytes_nn, ptrs, owner=latents)
        enc.run(); enc.wait()
        cc = enc.bytes(0)
        with open(a.out, "wb") as f:
            f.write(prefix + cc)
        # what was written decodes to the planes the last evaluation scored
        h2 = writer.parse_cc_header(cc)
        p, q = h2.n_bytes_header, h2.n_bytes_header + h2.nn_n_bytes
        assert cc[p:q] == res.bytes_nn and list(h2.nn_q_step_log2) == list(res.header.nn_q_step_log2)
        back.add(cc[:p], cc[p:q], cc[q:], bitdepth, fdt)
        back.run(); back.wait()
        scored = [t.cpu().numpy() for t in ev.planes(0)]
        assert all(np.array_equal(x, y) for x, y in zip(back.planes(0), scored)), "the written stream does not decode to the evaluated planes"
    print(f"{a.out}: {len(prefix) + len(cc)} bytes (was {len(bs)})")
    dec.close()


if __name__ == "__main__":
    main()
