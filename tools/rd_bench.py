"""Times the evaluation of candidates from GIVEN latents (DecodeBatch.add_latents*, RdEvaluator)
against the route it replaces, in the same process: kodim14 alone and the 24 streams of `kodak24`.

  given_float_ms    the float path from device latents alone: one DecodeBatch of given slots, run + wait
  evaluate_ms       RdEvaluator.evaluate end to end: that run, the rate meter, the quality meter (PSNR), the host's float64 cost
  replaced_ms       what a caller did before: EncodeBatch.run -> bytes -> DecodeBatch.add -> run -> QualityMeter (PSNR)

  --ddeltas         instead of the above: the distortion deltas (DistortionDeltas) of the same sets -
                    passes of the float path per run, run + wait, the time per pass next to given_float_ms

Device times are event-timed on the stream the work runs on, after 3 warm-up runs, median of --runs.  Prints one JSON line.
The ingest kernel's own time comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/rd_bench.py --runs 3 --no-replaced"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from cool_chic_amd import DecodeBatch, EncodeBatch, RdEvaluator, synth, writer  # noqa: E402
from cool_chic_amd.quality import QualityMeter, _planes_to_frame_data  # noqa: E402


def event_ms(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def measure(streams, runs, replaced):
    st = torch.cuda.current_stream().cuda_stream
    n = len(streams)
    dec = DecodeBatch(0)
    for bs in streams:
        dec.add(*synth.split_image_stream(bs), 8, 0)
    dec.run(st)
    dec.wait(st)
    res = {"streams": n, "symbols": int(sum(dec.header(s).n_symbols for s in range(n)))}
    sources = [_planes_to_frame_data(dec.planes(s), 8, "rgb") for s in range(n)]  # the decoded frames themselves: SSE 0
    src_planes = [[torch.as_tensor(dec.plane_device(s, p), device="cuda").clone() for p in range(3)] for s in range(n)]

    given = DecodeBatch(0)
    ev = RdEvaluator(0)
    for s in range(n):
        given.add_latents_from(dec, s, bitdepth=8, frame_data_type=0)
        ev.add(dec.header(s), dec.network_bytes(s), dec.latent_ptrs(s), sources[s], owner=dec)

    def given_step():
        given.run(st)
        given.wait(st)

    res["given_float_ms"] = round(event_ms(given_step, runs), 3)
    for s in range(n):
        assert all(torch.equal(torch.as_tensor(given.plane_device(s, p), device="cuda"), src_planes[s][p]) for p in range(3)), s

    out = []

    def evaluate_step():
        out[:] = ev.evaluate(1e-3)

    res["evaluate_ms"] = round(event_ms(evaluate_step, runs), 3)
    assert all(sum(c.quality.sse) == 0 for c in out)
    res["model_bits"] = round(sum(c.rate.total_bits for c in out), 3)

    if replaced:
        enc = EncodeBatch(0)
        for s in range(n):
            enc.add_from_decode(dec, s)
        meter = QualityMeter(0)
        checked = []

        def replaced_step():
            enc.run(st)
            enc.wait(st)
            back = DecodeBatch(0)
            for s in range(n):
                cc = enc.bytes(s)
                h = writer.parse_cc_header(cc)
                p, q = h.n_bytes_header, h.n_bytes_header + h.nn_n_bytes
                back.add(cc[:p], cc[p:q], cc[q:], 8, 0)
            back.run(st)
            planes = [[torch.as_tensor(back.plane_device(s, p), device="cuda") for p in range(3)] for s in range(n)]
            q = meter.score_planes(planes, src_planes, [8] * n, ["rgb"] * n, ms_ssim=False)
            back.wait(st)
            checked[:] = [sum(x.sse) for x in q]
            back.close()

        res["replaced_ms"] = round(event_ms(replaced_step, runs), 3)
        assert checked == [0] * n
        res["replaced_over_evaluate"] = round(res["replaced_ms"] / res["evaluate_ms"], 1)
        meter.close()
        enc.close()
    ev.close()
    given.close()
    dec.close()
    return res


def measure_ddeltas(streams, runs, n_probe_slots):
    """Pass count and time of DistortionDeltas.run + wait over the streams' own latents, scored against the decoded frames."""
    from cool_chic_amd import DistortionDeltas

    st = torch.cuda.current_stream().cuda_stream
    n = len(streams)
    dec = DecodeBatch(0)
    for bs in streams:
        dec.add(*synth.split_image_stream(bs), 8, 0)
    dec.run(st)
    dec.wait(st)
    src_planes = [[torch.as_tensor(dec.plane_device(s, p), device="cuda").clone() for p in range(3)] for s in range(n)]
    given = DecodeBatch(0)
    dd = DistortionDeltas(0, n_probe_slots)
    for s in range(n):
        given.add_latents_from(dec, s, bitdepth=8, frame_data_type=0)
        dd.add(dec.header(s), dec.network_bytes(s), dec.latent_ptrs(s), [t.data_ptr() for t in src_planes[s]], 8, 0, owner=(dec, src_planes))

    def given_step():
        given.run(st)
        given.wait(st)

    def dd_step():
        dd.run(st)
        dd.wait(st)

    res = {"streams": n, "probe_slots": n_probe_slots, "passes": [dd.passes(s) for s in range(n)][:4], "passes_total": sum(dd.passes(s) for s in range(n))}
    res["given_float_ms"] = round(event_ms(given_step, runs), 3)
    res["ddeltas_ms"] = round(event_ms(dd_step, runs), 3)
    rounds = max(-(-dd.passes(s) // n_probe_slots) for s in range(n))
    res["rounds"] = rounds
    res["ms_per_pass"] = round(res["ddeltas_ms"] / res["passes_total"], 5)
    res["given_float_ms_per_frame"] = round(res["given_float_ms"] / n, 5)
    # every decoded frame is its own source: no move can lower the squared error
    m = torch.as_tensor(dd.delta_map(0, 0), device="cuda")
    assert int((m[m != -2 ** 63] < 0).sum()) == 0
    res["grid0_mean_dsse"] = round(float(m[m != -2 ** 63].double().mean()), 3)
    dd.close()
    given.close()
    dec.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--no-replaced", action="store_true", help="skip the replaced route (profiling runs)")
    ap.add_argument("--ddeltas", action="store_true", help="time the distortion deltas instead")
    ap.add_argument("--probe-slots", type=int, default=16)
    a = ap.parse_args()
    k24 = synth.workload("kodak24")["streams"]
    if a.ddeltas:
        print(json.dumps({"tool": "rd_bench --ddeltas", "runs": a.runs, "kodim14": measure_ddeltas(k24[:1], a.runs, a.probe_slots),
                          "kodak24": measure_ddeltas(k24, a.runs, a.probe_slots)}))
        return
    print(json.dumps({"tool": "rd_bench", "runs": a.runs, "kodim14": measure(k24[:1], a.runs, not a.no_replaced),
                      "kodak24": measure(k24, a.runs, not a.no_replaced)}))


if __name__ == "__main__":
    main()
