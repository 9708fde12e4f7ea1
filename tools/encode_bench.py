"""Times the device writer (EncodeBatch) against the host writer and against decoding:
kodim14 alone, the 24 streams of `kodak24` in one run, one 4K stream.  Device times are event-timed on the stream the work
runs on, after warm-up runs, median of --runs; host times are wall clock of the same process.  Prints one JSON line.

Per-kernel times (contexts / chain) come from a run of their own:
    rocprofv3 --kernel-trace --stats -- python tools/encode_bench.py --runs 3 --no-host
--measure adds the rate meter (EncodeBatch.measure + wait, with and without the map) on the same handles.
--deltas adds the rate sensitivity maps (EncodeBatch.measure_deltas + wait) beside measure + wait on the same handles and
prints their ratio next to the count of ARM evaluations per pixel it is made of."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from cool_chic_amd import DecodeBatch, EncodeBatch, synth, writer  # noqa: E402


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


def decoded(streams, bitdepth=8):
    dec = DecodeBatch(0)
    for bs in streams:
        hdr, nn, lat = synth.split_image_stream(bs)
        dec.add(hdr, nn, lat, bitdepth, 0)
    dec.run()
    dec.wait()
    return dec


def measure(streams, runs, host, rate=False, deltas=False):
    st = torch.cuda.current_stream().cuda_stream
    dec = decoded(streams)
    n_sym = sum(dec.header(s).n_symbols for s in range(len(streams)))
    res = {"streams": len(streams), "symbols": int(n_sym)}

    def dec_step():
        dec.run(st)
        dec.wait(st)

    res["decode_ms"] = round(event_ms(dec_step, runs), 3)
    enc = EncodeBatch(0)
    for s in range(len(streams)):
        enc.add_from_decode(dec, s)

    def enc_step():
        enc.run(st)
        enc.wait(st)

    res["device_encode_ms"] = round(event_ms(enc_step, runs), 3)
    for s, bs in enumerate(streams):
        assert enc.bytes(s) == b"".join(synth.split_image_stream(bs)), s
    res["device_ns_per_symbol"] = round(res["device_encode_ms"] * 1e6 / n_sym, 2)
    if rate:  # the rate meter on the same handle: measure() + wait(), without and with the per-latent map
        for key, want_map in (("measure_ms", False), ("measure_map_ms", True)):
            def rate_step():
                enc.measure(st, rate_map=want_map)
                enc.wait(st)

            res[key] = round(event_ms(rate_step, runs), 3)
        words = sum(int(enc.slot_status(s)[1][1]) for s in range(len(streams)))
        res["model_bits"] = round(sum(enc.rate(s).total_bits for s in range(len(streams))), 3)
        res["payload_bits"] = 32 * words
        res["run_over_measure"] = round(res["device_encode_ms"] / res["measure_ms"], 1)
    if deltas:  # measure_deltas() + wait() beside measure() + wait(), same handle, same inputs
        def meter_step():
            enc.measure(st)
            enc.wait(st)

        def deltas_step():
            enc.measure_deltas(st)
            enc.wait(st)

        res["measure_ms"] = round(event_ms(meter_step, runs), 3)
        res["measure_deltas_ms"] = round(event_ms(deltas_step, runs), 3)
        res["deltas_over_measure"] = round(res["measure_deltas_ms"] / res["measure_ms"], 1)
        # ARM evaluations per pixel as launched: the meter's 1, own + 3 per spatial tap, base + 2 per IFCE source on the
        # grids that have sources (an upper count: taps cut by a border are not evaluated)
        evals = 0
        for s in range(len(streams)):
            h = dec.header(s)
            for g in range(h.n_grids):
                fin = h.input_features_ifce[g] if g != h.n_grids - 1 else 0
                evals += h.grid_h[g] * h.grid_w[g] * (2 + 3 * h.spatial_context_arm + ((1 + 2 * fin) if fin else 0))
        res["arm_evaluations_per_symbol"] = round(evals / n_sym, 1)
    if host:
        jobs = []
        for s in range(len(streams)):
            h = dec.header(s)
            jobs.append((h, dec.network_bytes(s), [dec.latent(s, g) for g in range(h.n_grids)]))
        t = []
        for _ in range(3 if n_sym < 2e6 else 1):
            t0 = time.perf_counter()
            for h, nn, lat in jobs:  # one thread, one stream after the other: what ccd_encode_coolchic costs
                writer.encode_coolchic(h, nn, lat)
            t.append((time.perf_counter() - t0) * 1e3)
        res["host_encode_ms"] = round(statistics.median(t), 1)
        res["host_over_device"] = round(res["host_encode_ms"] / res["device_encode_ms"], 1)
    res["encode_over_decode"] = round(res["device_encode_ms"] / res["decode_ms"], 2)
    enc.close()
    dec.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--no-host", action="store_true", help="skip the host writer (profiling runs)")
    ap.add_argument("--no-4k", action="store_true")
    ap.add_argument("--measure", action="store_true", help="also time the rate meter (EncodeBatch.measure) beside every run")
    ap.add_argument("--deltas", action="store_true", help="also time the rate sensitivity maps (EncodeBatch.measure_deltas) beside measure")
    a = ap.parse_args()
    k24 = synth.workload("kodak24")["streams"]
    out = {"tool": "encode_bench", "runs": a.runs,
           "kodim14": measure(k24[:1], a.runs, not a.no_host, a.measure, a.deltas),
           "kodak24": measure(k24, a.runs, not a.no_host, a.measure, a.deltas)}
    if not a.no_4k:
        out["uhd4k_one"] = measure([synth.image_stream(2160, 3840)], a.runs, not a.no_host, a.measure, a.deltas)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
