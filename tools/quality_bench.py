"""Times the quality meter (cool_chic_amd/quality.py, csrc/ccd_quality.hip) on the kodak24 set.

The 24 streams of synth.kodak24() are decoded once; the sources are the decoded planes plus seeded noise, resident in HBM.
A scoring (enqueue + finish, i.e. including the copy of the results to the host) is timed with device events after a
warm-up, PSNR alone and PSNR + MS-SSIM.  Next to the time the tool prints the bytes and floating-point operations the
algorithm needs, computed from the shapes, the time the MI355X would need for each at its peak rate, and which of the
two is the larger (the bound)."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from cool_chic_amd import DecodeBatch, synth  # noqa: E402
from cool_chic_amd.quality import QualityMeter, scratch_bytes  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s (MI355X specification)
F64_VECTOR_PEAK = 78.6e12  # flop / s: the window pass accumulates in float64 on the vector ALUs


def algorithmic_work(shapes, ms_ssim):
    """(bytes, flops) for planes [(h, w, bytes per sample)]: what the definitions need, not what the kernels happen to do."""
    nbytes = flops = 0
    for h, w, bps in shapes:
        nbytes += 2 * h * w * bps          # squared error: both pictures once
        flops += 3 * h * w                 # subtract, multiply, add
        if not ms_ssim or min(h, w) < 176:
            continue
        for j in range(5):
            hj, wj = h >> j, w >> j
            nbytes += 2 * hj * wj * (bps if j == 0 else 4)          # both pictures of the scale read once
            if j < 4:
                nbytes += 2 * (hj // 2) * (wj // 2) * 4 * 1         # the pooled pictures written once
                flops += 2 * (hj // 2) * (wj // 2) * 3
            pos = (hj - 10) * (wj - 10)
            # five maps, two separable passes of 11 multiply-adds; three products; about 20 operations for cs and ssim
            flops += pos * (5 * 2 * 11 * 2 + 3 + 20)
    return nbytes, flops


def timed(meter, dec, src, bitdepths, ms_ssim, warmup, min_seconds):
    for _ in range(warmup):
        meter.score_planes(dec, src, bitdepths, ms_ssim=ms_ssim)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, total_ms = 0, 0.0
    while total_ms < min_seconds * 1e3:
        n = 20
        e0.record()
        for _ in range(n):
            meter.score_planes(dec, src, bitdepths, ms_ssim=ms_ssim)
        e1.record()
        e1.synchronize()
        total_ms += e0.elapsed_time(e1)
        reps += n
    return total_ms / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0, help="length of each timed window")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "quality_bench needs the MI355X"
    streams, sizes = synth.kodak24()
    batch = DecodeBatch(0)
    for bs in streams:
        batch.add(*synth.split_image_stream(bs), 8, 0)
    batch.run()
    batch.wait()
    dec = []
    for slot in range(len(streams)):
        dec.append([torch.as_tensor(batch.plane_device(slot, p), device="cuda:0").clone() for p in range(3)])
    torch.cuda.synchronize()
    batch.close()
    gen = torch.Generator(device="cuda:0").manual_seed(1234)
    src = [[(p.to(torch.int16) + torch.randint(-6, 7, p.shape, generator=gen, device="cuda:0", dtype=torch.int16)).clamp(0, 255).to(torch.uint8)
            for p in planes] for planes in dec]
    bitdepths = [8] * len(dec)
    shapes = [(p.shape[0], p.shape[1], 1) for planes in dec for p in planes]
    geo = [([1] * 3, [1] * 3, pl[0].shape[0], pl[0].shape[1], pl[1].shape[0], pl[1].shape[1], 8) for pl in dec]
    out = {"workload": "kodak24", "frames": len(dec), "mpixel": sum(h * w for h, w, _ in shapes) / 3e6}
    with QualityMeter(0) as meter:
        q = meter.score_planes(dec, src, bitdepths)
        out["mean_psnr_db"] = sum(x.psnr_db for x in q) / len(q)
        out["mean_ms_ssim"] = sum(x.ms_ssim for x in q) / len(q)
        for name, ms_ssim in (("psnr", False), ("psnr_ms_ssim", True)):
            ms, reps = timed(meter, dec, src, bitdepths, ms_ssim, args.warmup, args.min_seconds)
            nbytes, flops = algorithmic_work(shapes, ms_ssim)
            t_mem, t_alu = nbytes / HBM_PEAK * 1e3, flops / F64_VECTOR_PEAK * 1e3
            out[name] = {"ms_per_scoring": ms, "scorings_timed": reps, "algorithmic_bytes": nbytes, "algorithmic_flops": flops,
                         "ms_at_peak_bandwidth": t_mem, "ms_at_peak_f64_rate": t_alu,
                         "bound": "memory" if t_mem >= t_alu else "compute", "share_of_bound": max(t_mem, t_alu) / ms,
                         "scratch_bytes": scratch_bytes(geo, 3 if ms_ssim else 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
