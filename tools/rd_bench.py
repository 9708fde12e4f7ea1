"""Times the evaluation of candidates from GIVEN latents (DecodeBatch.add_latents*, RdEvaluator)
against the route it replaces, in the same process: kodim14 alone and the 24 streams of `kodak24`.

  given_float_ms    the float path from device latents alone: one DecodeBatch of given slots, run + wait
  evaluate_ms       RdEvaluator.evaluate end to end: that run, the rate meter, the quality meter (PSNR), the host's float64 cost
  replaced_ms       what a caller did before: EncodeBatch.run -> bytes -> DecodeBatch.add -> run -> QualityMeter (PSNR)

  --ddeltas         instead of the above: the distortion deltas (DistortionDeltas) of the same sets -
                    passes of the float path per run, run + wait, the time per pass next to given_float_ms

  --rdoq            instead of the above: one requantisation step (RdoqStep) next to the
                    evaluate(rate_deltas, distortion_deltas) that feeds it, candidates and moves per step for three grid
                    masks; the same step in 1, 2, 4, 8 and 64 rounds (candidates, moves, open candidates, time); and for kodim14
                    the cost after 1, 2, 4, 8 steps of RdEvaluator.descend with rounds=1 and with rounds=8

  --inter           instead of the above: the distortion deltas of P / B frames (DistortionDeltas.add_inter, DESIGN.md section
                    4.15) - one P and one B frame of the `vid5` fixture and a 1080p B frame of synth.gop1080p, both roles: passes,
                    run + wait, the time per round split into float path, probe reconstruction and squared-error split (each
                    stage run alone through the library's measurement hook), next to K plain ccd_inter_reconstruct calls on the same frame

  --inter --joint   instead of the above: the requantisation descent of the same P / B frames (InterRdEvaluator.descend, DESIGN.md
                    section 4.15) run to its fixed point both ways, alternating the roles and with joint steps, from the same
                    latents (the stream's own with a seeded tenth moved by +-1, scored against the frame the own latents decode
                    to): evaluate() calls, distortion-delta runs, steps, moves, final D + lambda R and wall time of each way

  --dependents      instead of the above: the distortion deltas THROUGH the frames that predict from a moved one (DESIGN.md section
                    4.16) - the I frame of `vid5` and of synth.gop1080p(2) with their direct dependents: strides and passes with and
                    without the margin, run + wait beside the same candidate without dependents (median of 5, min, max), the
                    round's time split into float path, conversion, dep kernel and squared-error split, conflicts per grid

  --networks        instead of the above: the search over the networks' quantisation steps (NetworkQuantiser, DESIGN.md section
                    4.18) on a Kodak-size intra frame and on the 1080p I frame of gop1080p33, the stream's own networks dequantised,
                    the source the decoded frame plus seeded noise of +-3 LSB: wall time of one sweep per module (median of 5, min,
                    max), candidates per launch, device memory taken, the share of that spent building the candidates on the host, the same candidates (built outside the
                    timer) priced one at a time through RdEvaluator (one evaluator per candidate: add, evaluate, close) and the ratio; for the Kodak-size frame at three lambdas
                    the cost, network bytes and PSNR of the searched network beside the stream's own, and after descend(8)

  --networks --dependents  instead of the above: the search of an I frame's networks through the frames that predict from it
                    (NetworkQuantiser.search(dependents=...)) on the I frame of vid5 and on the 1080p I frame
                    of the 33-frame GOP, each with its direct dependents, against the same candidates priced one at a time.
  --networks --inter  instead of the above: the same search for the two cool-chics of a P / B frame (InterNetworkQuantiser, DESIGN.md
                    section 4.19) - the P frame of `vid5`, a 1080p P frame grown from it and a B frame of synth.gop1080p (--inter-sets): wall time of one sweep
                    per module and role (median of 5, min, max), candidates per launch, the host share spent building candidates, and
                    the same candidates (built outside the timer) one at a time through InterRdEvaluator (add, evaluate, close)

  --arm-refine      instead of the above: the ARM parameter table (EncodeBatch.measure_param_deltas) of
                    kodim14, of the 24 streams of `kodak24` in one handle and of the 1080p I frame of gop1080p33 (--refine-sets):
                    measure_param_deltas + wait for the whole table, event-timed and as wall time (3 warm-ups and the median of
                    --runs), in modes 0 (automatic: the incremental path) and 1 (generic); the
                    same candidates (built outside the timer) priced by the calls the parent commit has - one add_device slot
                    per candidate over the shared latents, measure, chunked by max_in_flight_bytes as NetworkQuantiser does -
                    and the ratio of the wall times; and one descent of 25 steps on kodim14 (ArmRefiner.refine)

  --ifce-refine     the same three inputs and figures for the IFCE parameter table (EncodeBatch.measure_ifce_deltas, DESIGN.md
                    section 4.21), and on kodim14 one RateRefiner descent of 25 steps (ARM + IFCE) beside ArmRefiner's 25 steps:
                    bits, bytes and wall time of both

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


def measure_rdoq(streams, runs, lmbda, trajectory):
    """The streams' own latents with a seeded tenth of the positions moved by +-1, scored against the frames the own latents
    decode to: the time of evaluate(rate_deltas, distortion_deltas), of one step over its maps (latents restored before every
    step, outside the timed region), candidates and moves for three masks, the step in 1 .. 64 rounds, and the cost along a
    descent with one round and with eight."""
    import numpy as np

    from cool_chic_amd import RdoqStep

    st = torch.cuda.current_stream().cuda_stream
    n = len(streams)
    dec = DecodeBatch(0)
    for bs in streams:
        dec.add(*synth.split_image_stream(bs), 8, 0)
    dec.run(st)
    dec.wait(st)
    sources = [_planes_to_frame_data(dec.planes(s), 8, "rgb") for s in range(n)]
    rng = np.random.default_rng(14)
    start, work = [], []
    ev = RdEvaluator(0)
    for s in range(n):
        h = dec.header(s)
        grids = []
        for g in range(h.n_grids):
            a = dec.latent(s, g).astype(np.int64)
            a = a + np.where(rng.random(a.shape) < 0.1, rng.choice([-1, 1], size=a.shape), 0)
            grids.append(torch.from_numpy(np.clip(a, -64, 63).astype(np.int8)).cuda())
        start.append(grids)
        work.append([t.clone() for t in grids])
        ev.add(h, dec.network_bytes(s), [t.data_ptr() for t in work[s]], sources[s], owner=work[s])
    n_grids = [dec.header(s).n_grids for s in range(n)]

    def restore():
        for a, b in zip(work, start):
            for t, u in zip(a, b):
                t.copy_(u)

    out = []

    def evaluate_step():
        out[:] = ev.evaluate(lmbda, rate_deltas=True, distortion_deltas=True)

    res = {"streams": n, "symbols": int(sum(dec.header(s).n_symbols for s in range(n))), "lmbda": lmbda}
    res["evaluate_deltas_ms"] = round(event_ms(evaluate_step, runs), 3)
    res["cost_before"] = [c.cost for c in out][:2]
    step = RdoqStep(0)
    kD, kR = [], []
    for s in range(n):
        step.add(dec.header(s), 0, [t.data_ptr() for t in work[s]], owner=work[s])
        step.set_maps(s, [ev.distortion_delta_map(s, g).__cuda_array_interface__["data"][0] for g in range(n_grids[s])],
                      [ev.rate_delta_map(s, g).__cuda_array_interface__["data"][0] for g in range(n_grids[s])], owner=ev)
        kD.append(1.0 / (3.0 * sources[s].n_pixels * 255.0 * 255.0))
        kR.append(lmbda / sources[s].n_pixels)

    def timed_step(masks, rounds):
        times = []
        for it in range(3 + runs):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step.step(kD, kR, [0.0] * n, masks, st, rounds=rounds)
            e1.record()
            step.wait(st)
            if it >= 3:
                times.append(e0.elapsed_time(e1))
        results = [step.result(s) for s in range(n)]
        return {"step_ms": round(statistics.median(times), 4), "step_ms_min_max": [round(min(times), 4), round(max(times), 4)],
                "candidates": sum(r.n_candidates for r in results), "moves": sum(r.n_moves for r in results),
                "open": sum(r.n_open for r in results), "d_cost_slot0": results[0].d_cost}

    all_masks = {"all_grids": [(1 << k) - 1 for k in n_grids], "grids_0_2": [7] * n, "grid_0": [1] * n}
    for label, masks in all_masks.items():
        res[label] = timed_step(masks, 1)
    for label in ("all_grids", "grids_0_2"):
        res[label + "_rounds"] = {str(r): timed_step(all_masks[label], r) for r in (1, 2, 4, 8, 64)}
    step.close()
    if trajectory:
        for rounds in (1, 8):
            restore()
            torch.cuda.synchronize()
            # coarse candidates own the raster: with every grid admitted a step is usually one move
            reports = ev.descend(lmbda, max_steps=8, grids=(0, 1, 2), rounds=rounds)
            last = ev.evaluate(lmbda)[0]
            costs = [rep[0].before.cost for rep in reports] + [last.cost]
            res["descent_grids_0_2" + ("" if rounds == 1 else f"_rounds{rounds}")] = {
                "cost_after_steps": {str(k): costs[k] for k in (0, 1, 2, 4, 8) if k < len(costs)},
                "moves_per_step": [rep[0].step.n_moves for rep in reports],
                "candidates_per_step": [rep[0].step.n_candidates for rep in reports],
                "open_per_step": [rep[0].step.n_open for rep in reports],
                "bits": [reports[0][0].before.bits, last.bits]}
    ev.close()
    dec.close()
    return res


def measure_inter(stream_bytes, coding_index, runs, n_probe_slots):
    """Both candidates of one P / B frame of a video stream, scored against the frame itself, its references as decode_video
    gives them."""
    import ctypes as C
    import os
    import tempfile

    from cool_chic_amd import DistortionDeltas
    from cool_chic_amd._lib import check, lib
    from cool_chic_amd.bitstream.decode import _split_frame, decode_video
    from cool_chic_amd.bitstream.header import VideoHeader
    from cool_chic_amd.bitstream.intercoding import _integer_planes

    st = torch.cuda.current_stream().cuda_stream
    vh = VideoHeader()
    rest = vh.read_header(stream_bytes)
    structure = vh.get_coding_structure()
    for k in range(coding_index + 1):
        fh, ccs, rest = _split_frame(rest)
    frame_type = "IPB".index(fh.get_value("frame_type"))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v.cool")
        with open(path, "wb") as f:
            f.write(stream_bytes)
        frames = decode_video(path)
    dev = torch.device("cuda:0")
    refs = [_integer_planes(frames[str(int(r))], dev) for r in structure[coding_index]["index_references"]][:frame_type]
    src = _integer_planes(frames[str(int(structure[coding_index]["display_order"]))], dev)
    h, w = src[0].shape
    gflow = (list(fh.get_value("global_flow")) + [0] * 4)[:4]
    bitdepth, fdt = fh.get_value("bitdepth"), ["rgb", "yuv420", "yuv444"].index(fh.get_value("frame_data_type"))
    stages = lib().ccd_dsens_debug_stages  # exported, not part of include/ccd.h: which stages of a round the next runs enqueue
    stages.restype, stages.argtypes = C.c_int, [C.c_void_p, C.c_int]
    taps = fh.get_value("warp_filter_size")
    dec = DecodeBatch(0)
    for ch, nn, lat in ccs:
        dec.add(ch.raw, nn, lat, 0, 0)
    dec.run(st); dec.wait(st)
    outs = [torch.as_tensor(dec.output_device(s), device="cuda") for s in range(2)]
    res = {"frame": "PB"[frame_type - 1], "size": [int(h), int(w)], "probe_slots": n_probe_slots, "warp_filter_size": int(taps)}

    def ptrs(planes):
        return (C.c_void_p * 3)(*[p.data_ptr() for p in planes])

    out_planes = [torch.empty_like(p) for p in src]

    def plain(n):  # the parent's entry point, n times: what a round of n probes would cost through it
        for _ in range(n):
            check(lib().ccd_inter_reconstruct(0, C.c_void_p(st or None), frame_type, h, w, bitdepth, fdt, C.c_void_p(outs[0].data_ptr()),
                                              C.c_void_p(outs[1].data_ptr()), ptrs(refs[0]), ptrs(refs[1]) if frame_type == 2 else None,
                                              (C.c_int32 * 4)(*gflow), taps, ptrs(out_planes)), "ccd_inter_reconstruct")

    res["plain_reconstruct_ms"] = round(event_ms(lambda: plain(1), runs), 4)
    res["plain_reconstruct_x_slots_ms"] = round(event_ms(lambda: plain(n_probe_slots), runs), 4)
    assert all(torch.equal(a, b) for a, b in zip(out_planes, src))
    for role, name in enumerate(("residue", "motion")):
        dd = DistortionDeltas(0, n_probe_slots)
        dd.add_inter(dec.header(role), dec.network_bytes(role), dec.latent_ptrs(role), [t.data_ptr() for t in src], bitdepth, fdt, frame_type, role,
                     outs[1 - role].data_ptr(), [t.data_ptr() for t in refs[0]], [t.data_ptr() for t in refs[1]] if frame_type == 2 else None,
                     gflow, taps, owner=(dec, src, refs, outs))

        def step():
            dd.run(st)
            dd.wait(st)

        passes = dd.passes(0)
        rounds = -(-passes // n_probe_slots)
        r = {"passes": passes, "rounds": rounds, "run_wait_ms": round(event_ms(step, runs), 3)}
        m = torch.as_tensor(dd.delta_map(0, 0), device="cuda")  # the frame is its own source: no move lowers the squared error
        assert int((m[m != -2 ** 63] < 0).sum()) == 0
        for label, mask in (("float_path", 1), ("probe_reconstruction", 2), ("sse", 4)):
            check(stages(dd._h, mask), "ccd_dsens_debug_stages")
            r[label + "_ms_per_round"] = round(event_ms(step, runs) / rounds, 5)
        check(stages(dd._h, 7), "ccd_dsens_debug_stages")
        r["ms_per_round"] = round(r["run_wait_ms"] / rounds, 5)
        r["plain_over_probe_reconstruction"] = round(res["plain_reconstruct_x_slots_ms"] / r["probe_reconstruction_ms_per_round"], 2)
        res[name] = r
        dd.close()
    dec.close()
    return res


def measure_dependents(stream_bytes, runs, n_probe_slots):
    """The I frame of a video stream as a candidate, alone and with the frames that predict from it directly as its dependents
    (DESIGN.md 4.16), scored against the frames the stream decodes to: passes with and without the margin per grid, run + wait of
    both handles (median, min, max), the round's time by stage, conflicts per grid."""
    import ctypes as C
    import os
    import tempfile

    from cool_chic_amd import DistortionDeltas
    from cool_chic_amd._lib import check, lib
    from cool_chic_amd.bitstream.decode import _split_frame, decode_video
    from cool_chic_amd.bitstream.header import VideoHeader
    from cool_chic_amd.bitstream.intercoding import _integer_planes
    from cool_chic_amd.dsens import dependent_margin, probe_stride

    st = torch.cuda.current_stream().cuda_stream
    vh = VideoHeader()
    rest = vh.read_header(stream_bytes)
    structure = vh.get_coding_structure()
    split = []
    for k in range(len(structure)):
        fh, ccs, rest = _split_frame(rest)
        split.append((fh, ccs))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v.cool")
        with open(path, "wb") as f:
            f.write(stream_bytes)
        frames = decode_video(path)
    dev = torch.device("cuda:0")
    planes = {int(d): _integer_planes(fd, dev) for d, fd in frames.items()}
    fh0, ccs0 = split[0]
    assert fh0.get_value("frame_type") == "I"
    display = int(structure[0]["display_order"])
    bitdepth, fdt = fh0.get_value("bitdepth"), ["rgb", "yuv420", "yuv444"].index(fh0.get_value("frame_data_type"))
    dec = DecodeBatch(0)
    dec.add(ccs0[0][0].raw, ccs0[0][1], ccs0[0][2], 0, 0)
    deps = []
    for k in range(1, len(structure)):
        refs = [int(r) for r in structure[k]["index_references"]]
        fh, ccs = split[k]
        n_refs = "IPB".index(fh.get_value("frame_type"))
        if display not in refs[:n_refs]:
            continue
        first = len(dec)
        for ch, nn, lat in ccs:
            dec.add(ch.raw, nn, lat, 0, 0)
        deps.append({"coding_index": k, "frame_type": n_refs, "which": refs[:n_refs].index(display), "slots": (first, first + 1),
                     "other": planes[refs[1 - refs[:n_refs].index(display)]] if n_refs == 2 else None,
                     "src": planes[int(structure[k]["display_order"])], "gflow": (list(fh.get_value("global_flow")) + [0] * 4)[:4],
                     "taps": int(fh.get_value("warp_filter_size"))})
    dec.run(st); dec.wait(st)
    arch, nn = dec.header(0), dec.network_bytes(0)
    src = planes[display]
    stages = lib().ccd_dsens_debug_stages  # exported, not part of include/ccd.h
    stages.restype, stages.argtypes = C.c_int, [C.c_void_p, C.c_int]

    def timed(dd):
        def step():
            dd.run(st)
            dd.wait(st)

        step(); step()
        torch.cuda.synchronize()
        out = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return step, {"median": round(statistics.median(out), 3), "min": round(min(out), 3), "max": round(max(out), 3)}

    m = dependent_margin(fdt, [d["taps"] for d in deps])
    res = {"size": [int(v) for v in src[0].shape], "probe_slots": n_probe_slots, "dependents": [d["coding_index"] for d in deps], "margin": m,
           "strides": {g: [probe_stride(arch, g, fdt), probe_stride(arch, g, fdt, margin=m)] for g in range(arch.n_grids)
                       if not arch.is_hyperlatent[g]}}
    alone = DistortionDeltas(0, n_probe_slots)
    alone.add(arch, nn, dec.latent_ptrs(0), [t.data_ptr() for t in src], bitdepth, fdt, owner=(dec, src))
    _, res["alone_run_wait_ms"] = timed(alone)
    res["alone_passes"] = alone.passes(0)
    own = [torch.as_tensor(alone.delta_map(0, g), device="cuda").clone() for g in range(arch.n_grids)]
    alone.close()
    dd = DistortionDeltas(0, n_probe_slots)
    dd.add(arch, nn, dec.latent_ptrs(0), [t.data_ptr() for t in src], bitdepth, fdt, owner=(dec, src))
    outs = []
    for d in deps:
        o = [torch.as_tensor(dec.output_device(s), device="cuda") for s in d["slots"]]
        outs.append(o)
        dd.add_dependent(0, d["frame_type"], d["which"], o[0].data_ptr(), o[1].data_ptr(), [t.data_ptr() for t in d["src"]],
                         None if d["other"] is None else [t.data_ptr() for t in d["other"]], d["gflow"], d["taps"], owner=(o, planes))
    step, res["run_wait_ms"] = timed(dd)
    res["passes"] = dd.passes(0)
    rounds = -(-res["passes"] // n_probe_slots)
    res["rounds"] = rounds
    res["conflicts"] = [dd.dep_conflicts(0, g) for g in range(arch.n_grids)]
    assert all(torch.equal(torch.as_tensor(dd.delta_map(0, g), device="cuda"), own[g]) for g in range(arch.n_grids))
    # every frame is its own source and the base planes are the decoded ones: no move lowers a dependent's squared error
    dm = torch.as_tensor(dd.dep_delta_map(0, 0), device="cuda")
    assert int((dm[dm != -2 ** 63] < 0).sum()) == 0
    for label, mask in (("float_path", 1), ("conversion", 8), ("dep_kernel", 16), ("sse", 4)):
        check(stages(dd._h, mask), "ccd_dsens_debug_stages")
        res[label + "_ms_per_round"] = round(event_ms(step, runs) / rounds, 5)
    check(stages(dd._h, 31), "ccd_dsens_debug_stages")
    res["ms_per_round"] = round(res["run_wait_ms"]["median"] / rounds, 5)
    dd.close()
    dec.close()
    return res


def measure_inter_descent(stream_bytes, coding_index, runs, lmbda, rounds, grids, max_steps):
    """InterRdEvaluator.descend on one P / B frame, alternating and joint, each from the same perturbed latents on a fresh
    evaluator: one unmeasured descent, then `runs` timed ones (host wall time around descend(), the device idle before and
    after)."""
    import os
    import tempfile
    import time

    import numpy as np

    from cool_chic_amd import InterRdEvaluator
    from cool_chic_amd.bitstream.decode import _split_frame, decode_video
    from cool_chic_amd.bitstream.header import VideoHeader

    vh = VideoHeader()
    rest = vh.read_header(stream_bytes)
    structure = vh.get_coding_structure()
    for k in range(coding_index + 1):
        fh, ccs, rest = _split_frame(rest)
    frame_type = fh.get_value("frame_type")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v.cool")
        with open(path, "wb") as f:
            f.write(stream_bytes)
        frames = decode_video(path)
    refs = [frames[str(int(r))] for r in structure[coding_index]["index_references"]][:"IPB".index(frame_type)]
    source = frames[str(int(structure[coding_index]["display_order"]))]
    dec = DecodeBatch(0)
    for ch, nn, lat in ccs:
        dec.add(ch.raw, nn, lat, 0, 0)
    dec.run(); dec.wait()
    rng = np.random.default_rng(14)
    start = []
    for s in range(2):
        row = []
        for g in range(dec.header(s).n_grids):
            a = dec.latent(s, g).astype(np.int64)
            a = a + np.where(rng.random(a.shape) < 0.1, rng.choice([-1, 1], size=a.shape), 0)
            row.append(torch.from_numpy(np.clip(a, -64, 63).astype(np.int8)).cuda())
        start.append(row)
    res = {"frame": frame_type, "size": [int(v) for v in source.img_size], "lmbda": lmbda, "rounds": rounds, "grids": grids, "max_steps": max_steps}
    for joint in (False, True):
        walls, r = [], {}
        for it in range(1 + runs):
            work = [[t.clone() for t in row] for row in start]
            ev = InterRdEvaluator(0)
            ev.add(frame_type, *[(dec.header(s), dec.network_bytes(s), [t.data_ptr() for t in work[s]]) for s in range(2)], refs,
                   fh.get_value("global_flow"), fh.get_value("warp_filter_size"), source, owner=work)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reports = ev.descend(lmbda, max_steps, grids=grids, rounds=rounds, joint=joint)
            torch.cuda.synchronize()
            if it > 0:
                walls.append((time.perf_counter() - t0) * 1e3)
            last = ev.evaluate(lmbda)[0]
            per_step = [sum(s.n_moves for s in rep[0].steps) if joint else rep[0].step.n_moves for rep in reports]
            idle = 1 if joint else 2
            now = {"evaluate_calls": len(reports), "dsens_runs": len(reports) * (2 if joint else 1), "steps": len(reports),
                   "moves": sum(per_step), "cost_before": reports[0][0].before.cost, "cost_after": last.cost,
                   "at_fixed_point": len(per_step) >= idle and not any(per_step[-idle:])}
            assert not r or now == r, "a descent is a function of its inputs"
            r = now
            ev.close()
        r["wall_ms"] = round(statistics.median(walls), 2)
        r["wall_ms_min_max"] = [round(min(walls), 2), round(max(walls), 2)]
        res["joint" if joint else "alternating"] = r
    dec.close()
    return res


def measure_follow(stream_bytes, runs, lmbda, rounds, grids, n_probe_slots):
    """The I frame of a video stream (a seeded tenth of its latents moved by +-1) with the frames that predict from it directly:
    one RDOQ step priced by own + dependent deltas, without follows and with claims that follow the flows -
    step time, moves and n_open of both, the reach launch, the flow-box launch and the round kernels timed apart, the evaluate
    that feeds the step, and the share of latents whose flow box exceeds the cells a lane walks, on the stream's flows and on
    random ones.  The dependents are held fixed (mask 0)."""
    import ctypes as C
    import os
    import tempfile

    import numpy as np

    from cool_chic_amd import RdoqStep, rdoq
    from cool_chic_amd._lib import check, lib
    from cool_chic_amd.bitstream.decode import _split_frame, decode_video
    from cool_chic_amd.bitstream.header import VideoHeader
    from cool_chic_amd.bitstream.intercoding import _integer_planes

    lane_cells = rdoq.lane_cells()
    st = torch.cuda.current_stream().cuda_stream
    vh = VideoHeader()
    rest = vh.read_header(stream_bytes)
    structure = vh.get_coding_structure()
    split = []
    for k in range(len(structure)):
        fh, ccs, rest = _split_frame(rest)
        split.append((fh, ccs))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v.cool")
        with open(path, "wb") as f:
            f.write(stream_bytes)
        frames = decode_video(path)
    dev = torch.device("cuda:0")
    planes = {int(d): _integer_planes(fd, dev) for d, fd in frames.items()}
    fh0, ccs0 = split[0]
    display = int(structure[0]["display_order"])
    fdt = ["rgb", "yuv420", "yuv444"].index(fh0.get_value("frame_data_type"))
    dec = DecodeBatch(0)
    dec.add(ccs0[0][0].raw, ccs0[0][1], ccs0[0][2], 0, 0)
    deps = []
    for k in range(1, len(structure)):
        refs = [int(r) for r in structure[k]["index_references"]]
        fh, ccs = split[k]
        n_refs = "IPB".index(fh.get_value("frame_type"))
        if display not in refs[:n_refs]:
            continue
        first = len(dec)
        for ch, nn, lat in ccs:
            dec.add(ch.raw, nn, lat, 0, 0)
        deps.append({"frame_type": n_refs, "which": refs[:n_refs].index(display), "slots": (first, first + 1),
                     "other": planes[refs[1 - refs[:n_refs].index(display)]] if n_refs == 2 else None,
                     "src": planes[int(structure[k]["display_order"])], "gflow": (list(fh.get_value("global_flow")) + [0] * 4)[:4],
                     "taps": int(fh.get_value("warp_filter_size"))})
    dec.run(st); dec.wait(st)
    arch, nn = dec.header(0), dec.network_bytes(0)
    rng = np.random.default_rng(14)
    start = []
    for g in range(arch.n_grids):
        a = dec.latent(0, g).astype(np.int64)
        a = a + np.where(rng.random(a.shape) < 0.1, rng.choice([-1, 1], size=a.shape), 0)
        start.append(torch.from_numpy(np.clip(a, -64, 63).astype(np.int8)).cuda())
    work = [t.clone() for t in start]
    source = frames[str(display)]
    ev = RdEvaluator(0, n_probe_slots)
    ev.add(arch, nn, [t.data_ptr() for t in work], source, owner=work)
    outs = []
    for d in deps:
        o = [torch.as_tensor(dec.output_device(s), device="cuda") for s in d["slots"]]
        outs.append(o)
        ev.add_dependent(0, d["frame_type"], d["which"], o[0].data_ptr(), o[1].data_ptr(), [t.data_ptr() for t in d["src"]],
                         None if d["other"] is None else [t.data_ptr() for t in d["other"]], d["gflow"], d["taps"], owner=(o, planes))

    def evaluate_step():
        ev.evaluate(lmbda, rate_deltas=True, distortion_deltas=True)

    res = {"size": [int(v) for v in source.img_size], "dependents": len(deps), "lmbda": lmbda, "rounds": rounds, "grids": grids, "lane_cells": lane_cells}
    res["evaluate_deltas_ms"] = round(event_ms(evaluate_step, min(runs, 3), warmup=1), 3)
    n_samples = sum(int(t.numel()) for t in planes[display])
    kD, kR = 1.0 / (n_samples * float(2 ** source.bitdepth - 1) ** 2), lmbda / source.n_pixels
    mask = sum(1 << g for g in grids if g < arch.n_grids)
    stages = lib().ccd_rdoq_debug_stages  # exported, not part of include/ccd.h
    stages.restype, stages.argtypes = C.c_int, [C.c_void_p, C.c_int]

    def ptr(a):
        return a.__cuda_array_interface__["data"][0]

    def handle(follow, motions=None):
        step = RdoqStep(0)
        step.add(arch, fdt, [t.data_ptr() for t in work], owner=work)
        step.set_maps(0, [ptr(ev.distortion_delta_map(0, g)) for g in range(arch.n_grids)], [ptr(ev.rate_delta_map(0, g)) for g in range(arch.n_grids)], owner=ev)
        step.set_dep_maps(0, [ptr(ev.dependent_delta_map(0, g)) for g in range(arch.n_grids)])
        zeros = []
        for k, d in enumerate(deps):  # the residue cool-chic of every dependent, held fixed: the raster the follow claims in
            h = dec.header(d["slots"][0])
            z = [torch.zeros((2, int(h.grid_h[g]), int(h.grid_w[g])), dtype=torch.float32, device="cuda") for g in range(h.n_grids)]
            zeros.append(z)
            slot = step.add(h, fdt, dec.latent_ptrs(d["slots"][0]), owner=dec)
            step.set_maps(slot, [None] * h.n_grids, [t.data_ptr() for t in z], owner=z)
            if follow:
                m = outs[k][1] if motions is None else motions[k]
                step.follow(0, d["frame_type"], d["which"], m.data_ptr(), target=slot, global_flow=d["gflow"], warp_filter_size=d["taps"], owner=m)
        n = 1 + len(deps)
        return step, ([kD] * n, [kR] * n, [0.0] * n, [mask] + [0] * len(deps))

    def timed(step, args, stage=7):
        check(stages(step._h, stage), "ccd_rdoq_debug_stages")
        times = []
        for it in range(3 + runs):
            for t, u in zip(work, start):
                t.copy_(u)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step.step(*args, st, rounds=rounds)
            e1.record()
            step.wait(st)
            if it >= 3:
                times.append(e0.elapsed_time(e1))
        check(stages(step._h, 7), "ccd_rdoq_debug_stages")
        return {"ms": round(statistics.median(times), 4), "min_max": [round(min(times), 4), round(max(times), 4)]}

    def share_big(step):
        big = total = 0
        for k in range(len(deps)):
            for g in range(arch.n_grids):
                b = torch.as_tensor(step.flow_boxes(0, k, g), device="cuda").to(torch.int64)
                cells = torch.clamp(b[..., 2] - b[..., 0] + 1, min=0) * torch.clamp(b[..., 3] - b[..., 1] + 1, min=0)
                big += int((cells > lane_cells).sum()); total += int(cells.numel())
        return round(big / max(total, 1), 4)

    for label, follow in (("without_follows", False), ("with_follows", True)):
        step, args = handle(follow)
        r = {"step": timed(step, args)}
        out = step.result(0)
        r.update(candidates=out.n_candidates, moves=out.n_moves, open=out.n_open, d_sse=out.d_sse, dep_sse=step.dep_sse(0))
        if follow:
            r["flow_box_over_lane_cells"] = share_big(step)
            r["reach"], r["flow_boxes"], r["rounds_and_sums"] = timed(step, args, 1), timed(step, args, 2), timed(step, args, 4)
        step.close()
        res[label] = r
    g = torch.Generator(device="cuda").manual_seed(14)
    motions = [(torch.rand(o[1].shape, generator=g, device="cuda") * 40.0 - 20.0).contiguous() for o in outs]
    step, args = handle(True, motions)
    r = {"step": timed(step, args)}
    out = step.result(0)
    r.update(moves=out.n_moves, open=out.n_open, flow_box_over_lane_cells=share_big(step))
    res["random_flows_20"] = r
    step.close()
    ev.close()
    dec.close()
    return res


def measure_networks(hdr, nn, payload, bitdepth, fdt, runs, lmbdas, descend_steps):
    """NetworkQuantiser.search on one intra cool-chic: the tables' wall times over `runs` searches at lmbdas[0], the yardstick
    (every feasible candidate of those tables through an RdEvaluator of its own) and, per lambda, what the search reached."""
    import time

    import numpy as np

    import cool_chic_amd
    from cool_chic_amd import NetworkQuantiser
    from cool_chic_amd.batch import FRAME_DATA_TYPES
    from cool_chic_amd.nnquant import MODULES, build_network

    dec = DecodeBatch(0)
    dec.add(hdr, nn, payload, bitdepth, fdt)
    dec.run(); dec.wait()
    arch = dec.header(0)
    rng = np.random.default_rng(18)
    maxv = 2 ** bitdepth - 1
    planes = [np.clip(p.astype(np.int64) + rng.integers(-3, 4, p.shape), 0, maxv).astype(p.dtype) for p in dec.planes(0)]
    source = _planes_to_frame_data(planes, bitdepth, FRAME_DATA_TYPES[fdt])
    latents = [torch.from_numpy(dec.latent(0, g)).cuda() for g in range(arch.n_grids)]
    ptrs = [t.data_ptr() for t in latents]
    dec.close()
    floats = writer.dequantise_network(arch, writer.network_values(arch, nn))
    res = {"size": [int(v) for v in arch.img_size], "symbols": int(arch.n_symbols), "parameters": int(floats.size), "runs": runs}
    cool_chic_amd.pool_trim(0)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    nq = NetworkQuantiser(0)
    searches = []
    for it in range(1 + runs):
        out = nq.search(arch, floats, ptrs, source, lmbdas[0], owner=latents)
        if it > 0:
            searches.append(out)
    torch.cuda.synchronize()
    res["device_mib_taken"] = round((free0 - torch.cuda.mem_get_info(0)[0]) / 2 ** 20, 1)  # the library's block cache after the searches
    one = searches[0]
    steps = [writer.q_step_range(g)[0] for g in range(8)]
    res["modules"] = {}
    for k, t in enumerate(one.tables):
        secs = [s.pricing[k].seconds for s in searches]
        build = [s.pricing[k].build_seconds for s in searches]
        _, gw, gb = next(m for m in MODULES if m[0] == t.module)
        nets = []
        for c in t.cells:
            if c.feasible:
                s = list(steps)
                s[gw], s[gb] = c.q_w, c.q_b
                nets.append(build_network(arch, floats, s))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for net in nets:  # the yardstick: one candidate at a time through the calls the parent commit has
            with RdEvaluator(0) as ev:
                ev.add(net.header, net.bytes_nn, ptrs, source, owner=latents)
                ev.evaluate(lmbdas[0])
        alone = time.perf_counter() - t0
        res["modules"][t.module] = {"candidates": len(t.cells), "feasible": len(nets), "per_launch": one.pricing[k].chunk,
                                    "sweep_s": {"median": round(statistics.median(secs), 4), "min": round(min(secs), 4), "max": round(max(secs), 4)},
                                    "of_which_building_candidates_s": round(statistics.median(build), 4),
                                    "one_at_a_time_s": round(alone, 4), "ratio": round(alone / statistics.median(secs), 2)}
        if t.chosen is not None:  # (a module without a feasible cell kept its steps)
            steps[gw], steps[gb] = t.cells[t.chosen].q_w, t.cells[t.chosen].q_b
    res["reached"] = {}
    for lmbda in lmbdas:
        out = nq.search(arch, floats, ptrs, source, lmbda, owner=latents)
        row = {}
        for label, a, b in (("stream", arch, nn), ("searched", out.header, out.bytes_nn)):
            work = [t.clone() for t in latents]
            with RdEvaluator(0) as ev:
                ev.add(a, b, [t.data_ptr() for t in work], source, owner=work)
                c = ev.evaluate(lmbda)[0]
                row[label] = {"cost": c.cost, "bytes_nn": len(b), "psnr_db": round(c.quality.psnr_db, 4), "bits": round(c.bits, 1)}
                if descend_steps > 0:
                    ev.descend(lmbda, descend_steps, grids=(0, 1, 2), rounds=8)
                    c = ev.evaluate(lmbda)[0]
                    row[label + f"_descend{descend_steps}"] = {"cost": c.cost, "psnr_db": round(c.quality.psnr_db, 4), "bits": round(c.bits, 1)}
        row["steps"] = list(out.header.nn_q_step_log2)
        res["reached"][repr(lmbda)] = row
    return res


def measure_network_dependents(stream_bytes, runs, lmbdas):
    """NetworkQuantiser.search(dependents=...) on the first I frame of a video stream with its direct dependents:
    the tables' wall times over `runs` searches at lmbdas[0]; the yardstick - the same candidates one at a time through calls the
    parent commit has, RdEvaluator for the frame, ccd_inter_reconstruct + QualityMeter per dependent, candidates built outside the
    timer; the kernel time of one reference item next to one motion item of a P and of a B dependent; per lambda the summed
    cost (the frame and its direct dependents) of the networks chosen without and with the dependents."""
    import ctypes as C
    import os
    import tempfile
    import time

    import numpy as np

    from cool_chic_amd import InterScore, NetworkQuantiser
    from cool_chic_amd._lib import check, lib
    from cool_chic_amd.batch import FRAME_DATA_TYPES
    from cool_chic_amd.bitstream.decode import _split_frame, decode_video
    from cool_chic_amd.bitstream.header import VideoHeader
    from cool_chic_amd.bitstream.intercoding import _integer_planes
    from cool_chic_amd.nnquant import MODULES, Dependent, build_network
    from cool_chic_amd.quality import QualityMeter, _frame_planes
    from cool_chic_amd.rd import cost_with_dependents

    st = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda:0")
    vh = VideoHeader()
    rest = vh.read_header(stream_bytes)
    structure = vh.get_coding_structure()
    split = []
    for _ in range(len(structure)):
        fh, ccs, rest = _split_frame(rest)
        split.append((fh, ccs))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v.cool")
        with open(path, "wb") as f:
            f.write(stream_bytes)
        frames = decode_video(path)
    fh0, ccs0 = split[0]
    assert fh0.get_value("frame_type") == "I"
    display = int(structure[0]["display_order"])
    bitdepth, fdt = fh0.get_value("bitdepth"), FRAME_DATA_TYPES.index(fh0.get_value("frame_data_type"))
    maxv = 2 ** bitdepth - 1
    rng = np.random.default_rng(22)

    def noisy(fd):  # the decoded frame plus seeded noise of a few LSB, as measure_networks' source
        return _planes_to_frame_data([np.clip(p.astype(np.int64) + rng.integers(-3, 4, p.shape), 0, maxv).astype(p.dtype) for p in fd.integer_planes()],
                                     bitdepth, FRAME_DATA_TYPES[fdt])

    dec = DecodeBatch(0)
    dec.add(ccs0[0][0].raw, ccs0[0][1], ccs0[0][2], bitdepth, fdt)
    found = []
    for k in range(1, len(structure)):
        refs = [int(r) for r in structure[k]["index_references"]]
        fh, ccs = split[k]
        n_refs = "IPB".index(fh.get_value("frame_type"))
        if display not in refs[:n_refs]:
            continue
        first = len(dec)
        for ch, nn, lat in ccs:
            dec.add(ch.raw, nn, lat, 0, 0)
        found.append((k, fh, n_refs, refs[:n_refs], first))
    dec.run(st); dec.wait(st)
    arch, nn = dec.header(0), dec.network_bytes(0)
    latents = [torch.from_numpy(dec.latent(0, g)).cuda() for g in range(arch.n_grids)]
    ptrs = [t.data_ptr() for t in latents]
    source = noisy(frames[str(display)])
    deps, keep = [], []
    for k, fh, n_refs, refs, first in found:
        which = refs.index(display)
        outs = [torch.as_tensor(dec.output_device(first + j), device=dev)[0].clone() for j in range(2)]
        other = _integer_planes(frames[str(refs[1 - which])], dev) if n_refs == 2 else None
        d_source = noisy(frames[str(int(structure[k]["display_order"]))])
        keep.append((outs, other, _frame_planes(d_source, dev)))
        deps.append(Dependent(n_refs, which, outs[0].data_ptr(), outs[1].data_ptr(), None if other is None else [t.data_ptr() for t in other],
                              (list(fh.get_value("global_flow")) + [0] * 4)[:4], int(fh.get_value("warp_filter_size")), d_source, owner=keep[-1]))
    dec.close()
    H, W = int(arch.img_size[0]), int(arch.img_size[1])
    floats = writer.dequantise_network(arch, writer.network_values(arch, nn))
    res = {"size": [H, W], "dependents": len(deps), "of_which_B": sum(d.frame_type == 2 for d in deps), "runs": runs}

    def ptrs3(planes):
        return (C.c_void_p * 3)(*[p.data_ptr() for p in planes])

    def reconstruct(d, src_planes, planes, out):  # ccd_inter_reconstruct of a dependent against `planes`
        refs = [planes, planes]
        if d.frame_type == 2:
            refs[1 - d.which] = None
        r = [ptrs3(x) if x is not None else (C.c_void_p * 3)(*d.other_ref_ptrs) for x in refs]
        check(lib().ccd_inter_reconstruct(0, C.c_void_p(st or None), d.frame_type, H, W, bitdepth, fdt, C.c_void_p(d.residue_ptr), C.c_void_p(d.motion_ptr),
                                          r[0], r[1] if d.frame_type == 2 else None, (C.c_int32 * 4)(*d.global_flow), d.warp_filter_size, ptrs3(out)),
              "ccd_inter_reconstruct")

    nq = NetworkQuantiser(0)
    searches = []
    for it in range(1 + runs):
        out = nq.search(arch, floats, ptrs, source, lmbdas[0], owner=latents, dependents=deps)
        if it > 0:
            searches.append(out)
    one = searches[0]
    steps = [writer.q_step_range(g)[0] for g in range(8)]
    res["modules"] = {}
    scratch = [torch.empty_like(p) for p in keep[0][2]]
    for k, t in enumerate(one.tables):
        secs = [s.pricing[k].seconds for s in searches]
        _, gw, gb = next(m for m in MODULES if m[0] == t.module)
        nets = []
        for c in t.cells:
            if c.feasible:
                s = list(steps)
                s[gw], s[gb] = c.q_w, c.q_b
                nets.append(build_network(arch, floats, s))
        moving = t.module in ("upsampling", "synthesis")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with QualityMeter(0) as meter:
            for net in nets:  # the yardstick: one candidate at a time through the calls the parent commit has
                with RdEvaluator(0) as ev:
                    ev.add(net.header, net.bytes_nn, ptrs, source, owner=latents)
                    ev.evaluate(lmbdas[0])
                    if moving:  # (a candidate that moves no plane keeps the current dependent term on both routes)
                        planes = ev.planes(0)
                        for d, (_, _, d_src) in zip(deps, keep):
                            reconstruct(d, d_src, planes, scratch)
                            meter.score_planes([scratch], [d_src], [bitdepth], ms_ssim=False)
        alone = time.perf_counter() - t0
        res["modules"][t.module] = {"candidates": len(t.cells), "feasible": len(nets), "per_launch": one.pricing[k].chunk,
                                    "sweep_s": {"median": round(statistics.median(secs), 4), "min": round(min(secs), 4), "max": round(max(secs), 4)},
                                    "one_at_a_time_s": round(alone, 4), "ratio": round(alone / statistics.median(secs), 2)}
        if t.chosen is not None:
            steps[gw], steps[gb] = t.cells[t.chosen].q_w, t.cells[t.chosen].q_b

    # one reference item next to one motion item (mode 2) of the same frame: a run with N items less a run with none, over N
    own_planes = _frame_planes(source, dev)
    res["item_ms"] = {}
    n_items = 16
    for label, ft in (("P", 1), ("B", 2)):
        pick = [(d, kp) for d, kp in zip(deps, keep) if d.frame_type == ft]
        if not pick:
            continue
        d, (_, _, d_src) = pick[0]
        o = [t.data_ptr() for t in own_planes]
        refs = [o, o]
        if ft == 2:
            refs[1 - d.which] = list(d.other_ref_ptrs)

        def timed(kind):
            with InterScore(0) as score:
                score.add_frame(ft, H, W, bitdepth, fdt, d.residue_ptr, d.motion_ptr, refs[0], refs[1] if ft == 2 else None,
                                [t.data_ptr() for t in d_src], d.global_flow, d.warp_filter_size)
                for _ in range(n_items if kind else 0):
                    if kind == "motion":
                        score.add(0, 1, d.motion_ptr)
                    elif kind == "residue":
                        score.add(0, 0, d.residue_ptr)
                    elif kind == "both":
                        score.add_refs(0, o, o)
                    else:
                        score.add_refs(0, o if d.which == 0 else None, o if d.which == 1 else None)

                def step():
                    score.run(st)
                    score.wait(st)
                return event_ms(step, runs)
        base = timed(None)
        row = {"run_without_items_ms": round(base, 4)}
        for kind in ("motion", "residue", "ref") + (("both",) if ft == 2 else ()):
            row[kind + "_item_ms"] = round((timed(kind) - base) / n_items, 4)
        res["item_ms"][label] = row

    def summed(net):
        """cost_with_dependents of a search result: its own candidate and the dependents against its planes."""
        with RdEvaluator(0) as ev, QualityMeter(0) as meter:
            ev.add(net.header, net.bytes_nn, ptrs, source, owner=latents)
            c = ev.evaluate(lmbda)[0]
            terms = []
            for d, (_, _, d_src) in zip(deps, keep):
                reconstruct(d, d_src, ev.planes(0), scratch)
                r = meter.score_planes([scratch], [d_src], [bitdepth], ms_ssim=False)[0]
                terms.append((tuple(int(v) for v in r.sse), tuple(int(v) for v in r.n), bitdepth))
            return c.cost, cost_with_dependents((c.mse, c.bits, c.cost), terms)

    res["reached"] = {}
    for lmbda in lmbdas:
        row = {}
        for label, kw in (("without", {}), ("with", {"dependents": deps})):
            out = nq.search(arch, floats, ptrs, source, lmbda, owner=latents, **kw)
            own, total = summed(out)
            row[label] = {"steps": list(out.header.nn_q_step_log2), "bytes_nn": len(out.bytes_nn), "own_cost": own, "summed_cost": total}
        res["reached"][repr(lmbda)] = row
    return res


def measure_arm_table(ccs, runs, warmup, descent_steps, ifce=False):
    """The ARM parameter table (ifce: the IFCE parameter table) of the cool-chics `ccs` [(header bytes, NN payload, latent payload)] in one
    handle."""
    import time

    import numpy as np

    from cool_chic_amd._lib import CCHeader
    from cool_chic_amd.nnquant import NetworkQuantiser
    from cool_chic_amd.nnrefine import ArmRefiner, RateRefiner

    st = torch.cuda.current_stream().cuda_stream
    dec = DecodeBatch(0)
    for hdr, nn, payload in ccs:
        dec.add(hdr, nn, payload, 0, 0)
    dec.run(st); dec.wait(st)
    n = len(ccs)
    archs = [dec.header(s) for s in range(n)]
    nns = [dec.network_bytes(s) for s in range(n)]
    ptrs = [dec.latent_ptrs(s) for s in range(n)]
    first = [sum(writer.network_layout(a)[:2]) if ifce else 0 for a in archs]          # the table's row 0 in writer.network_values
    n_arm = [sum(writer.network_layout(a)[2:4] if ifce else writer.network_layout(a)[:2]) for a in archs]  # rows of the table
    res = {"streams": n, "symbols": int(sum(a.n_symbols for a in archs)), "candidates": 2 * sum(n_arm), "runs": runs, "warmup": warmup}
    enc = EncodeBatch(0)
    for s in range(n):
        enc.add_device(archs[s], nns[s], ptrs[s], owner=dec)
    for mode in (0, 1):  # automatic (the incremental path where the state fits the LDS) and generic
        def table():
            (enc.measure_ifce_deltas if ifce else enc.measure_param_deltas)(st, mode=mode)
            enc.wait(st)
        for _ in range(warmup):
            table()
        torch.cuda.synchronize()
        ev_ms, wall = [], []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            table()
            e1.record()
            e1.synchronize()
            wall.append(time.perf_counter() - t0)
            ev_ms.append(e0.elapsed_time(e1))
        res[f"table_mode{mode}"] = {"event_ms": {"median": round(statistics.median(ev_ms), 2), "min": round(min(ev_ms), 2), "max": round(max(ev_ms), 2)},
                                    "wall_s": round(statistics.median(wall), 4)}
    tables = [(enc.ifce_deltas if ifce else enc.param_deltas)(s) for s in range(n)]
    base = [enc.rate(s).total_bits for s in range(n)]
    enc.close()
    # the yardstick: every candidate a slot of its own over the shared latents; the candidates are built OUTSIDE the timer
    nq = NetworkQuantiser(0)
    yard, worst = 0.0, 0.0
    for s in range(n):
        values = writer.network_values(archs[s], nns[s])
        cands = []
        for k in range(n_arm[s]):
            for sign in (-1, 1):
                v = values.copy()
                v[first[s] + k] += sign
                h = CCHeader.from_buffer_copy(bytes(archs[s]))
                cands.append((h, writer.encode_network(h, v)))
        chunk = nq.chunk_size(archs[s], 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bits = []
        for at in range(0, len(cands), chunk):
            with EncodeBatch(0) as one:
                for h, b in cands[at:at + chunk]:
                    one.add_device(h, b, ptrs[s], owner=dec)
                one.measure(st)
                one.wait(st)
                bits += [one.rate(i).total_bits for i in range(len(cands[at:at + chunk]))]
        yard += time.perf_counter() - t0
        got = np.asarray(bits).reshape(-1, 2) - base[s]  # two rounded totals apart: a plausibility check, not the accuracy test
        worst = max(worst, float(np.abs(got - tables[s].bits).max(initial=0.0)))
        res.setdefault("yardstick_per_launch", chunk)
    res["yardstick_wall_s"] = round(yard, 4)
    res["ratio_yardstick_over_table_mode0"] = round(yard / res["table_mode0"]["wall_s"], 2)
    res["ratio_table_mode1_over_mode0"] = round(res["table_mode1"]["wall_s"] / res["table_mode0"]["wall_s"], 2)
    res["largest_difference_from_the_yardstick_bits"] = worst
    if descent_steps > 0:
        for key, refiner in (("descent", ArmRefiner(0)),) + ((("descent_arm_ifce", RateRefiner(0)),) if ifce else ()):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fine = refiner.refine(archs[0], writer.network_values(archs[0], nns[0]), ptrs[0], descent_steps, owner=dec)
            n_first = sum(writer.network_layout(archs[0])[:2])
            res[key] = {"steps": len(fine.log), "stopped": fine.stopped, "wall_s": round(time.perf_counter() - t0, 3),
                        "objective_before": fine.start_objective, "objective_after": fine.log[-1].objective if fine.log else fine.start_objective,
                        "total_bits_after": fine.log[-1].total_bits if fine.log else None,
                        "bytes_nn_before": len(nns[0]), "bytes_nn_after": len(fine.bytes_nn),
                        "ifce_moves": sum(m.index >= n_first for step in fine.log for m in step.moves)}
    dec.close()
    return res


def ip_1080p():
    """A 1920x1080 I P stream in the geometry of gop1080p33, whose own structure (two I frames, hierarchical B between them) has
    no P frame: the I and P frames of `vid5` grown the way synth.gop1080p grows its donors."""
    from cool_chic_amd.bitstream.decode import _split_frame
    from cool_chic_amd.bitstream.header import VideoHeader

    H, W = 1080, 1920
    bs, z = synth._golden("vid5")
    rest = VideoHeader().read_header(bs)
    out, cc_idx = [writer.video_header_bytes(2, [0], [1])], 0
    for k in range(2):
        fh, ccs, rest = _split_frame(rest)
        assert fh.get_value("frame_type") == "IP"[k]
        refs = [0] * k
        out.append(writer.frame_header_bytes(k, "IP"[k], fh.c.frame_data_type, fh.c.bitdepth, refs, [0] * (2 * len(refs)), fh.c.warp_filter_size))
        for ch, nn, _ in ccs:
            donor = writer.parse_cc_header(ch.raw)
            lat = [z[f"cc{cc_idx}.latent{g}"] for g in range(donor.n_grids)]
            if donor.latent_resolution[0] == 0:  # residue / intra: "auto" levels for this picture size
                v = synth.auto_resolution(H * W)
                arch = writer.derive_arch(donor, img_size=(H, W), latent_resolution=(0, v),
                                          hyperlatent_resolution=(4, v) if donor.flag_hyperlatent else tuple(donor.hyperlatent_resolution),
                                          n_latent_grids=(v + 1) + ((v - 3) if donor.flag_hyperlatent else 0))
                nn = writer.encode_network(arch, writer.adapt_network(donor, z[f"cc{cc_idx}.nn_ints"], arch))
            else:                                # motion: latent 2-6 whatever the size
                arch = writer.derive_arch(donor, img_size=(H, W))
            out.append(writer.encode_coolchic(arch, nn, writer.tile_latents(lat, donor, arch)))
            cc_idx += 1
    return b"".join(out)


def measure_inter_networks(stream_bytes, coding_index, runs, lmbda):
    """InterNetworkQuantiser.search on one P / B frame of a video stream (the stream's own networks dequantised, the source the
    decoded frame plus seeded noise of +-3 LSB, the references as decode_video gives them): the tables' wall times over `runs`
    searches and the yardstick - every feasible candidate of those tables, built outside the timer, through an InterRdEvaluator
    of its own (add, evaluate, close)."""
    import os
    import tempfile
    import time

    import numpy as np

    from cool_chic_amd import InterRdEvaluator
    from cool_chic_amd.bitstream.decode import _split_frame, decode_video
    from cool_chic_amd.bitstream.header import VideoHeader
    from cool_chic_amd.bitstream.intercoding import _integer_planes
    from cool_chic_amd.nnquant import MODULES, build_network
    from cool_chic_amd.nnquant_inter import ROLES, InterNetworkQuantiser

    vh = VideoHeader()
    rest = vh.read_header(stream_bytes)
    structure = vh.get_coding_structure()
    for k in range(coding_index + 1):
        fh, ccs, rest = _split_frame(rest)
    frame_type = fh.get_value("frame_type")
    n_refs = "IPB".index(frame_type)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v.cool")
        with open(path, "wb") as f:
            f.write(stream_bytes)
        frames = decode_video(path)
    dev = torch.device("cuda:0")
    refs = [_integer_planes(frames[str(int(r))], dev) for r in structure[coding_index]["index_references"]][:n_refs]
    own = frames[str(int(structure[coding_index]["display_order"]))]
    rng = np.random.default_rng(18)
    maxv = 2 ** own.bitdepth - 1
    planes = [np.clip(p.astype(np.int64) + rng.integers(-3, 4, p.shape), 0, maxv).astype(p.dtype) for p in own.integer_planes()]
    source = _planes_to_frame_data(planes, own.bitdepth, own.frame_data_type)
    gflow, taps = fh.get_value("global_flow"), fh.get_value("warp_filter_size")
    dec = DecodeBatch(0)
    for ch, nn, lat in ccs:
        dec.add(ch.raw, nn, lat, 0, 0)
    dec.run(); dec.wait()
    archs = [dec.header(r) for r in range(2)]
    latents = [[torch.from_numpy(dec.latent(r, g)).cuda() for g in range(archs[r].n_grids)] for r in range(2)]
    ptrs = [[t.data_ptr() for t in row] for row in latents]
    dec.close()
    floats = [writer.dequantise_network(archs[r], writer.network_values(archs[r], ccs[r][1])) for r in range(2)]
    res = {"frame": frame_type, "size": [int(v) for v in archs[0].img_size], "warp_filter_size": int(taps),
           "parameters": [int(x.size) for x in floats], "runs": runs}
    nq = InterNetworkQuantiser(0)

    def search():
        return nq.search(frame_type, (archs[0], floats[0], ptrs[0]), (archs[1], floats[1], ptrs[1]), refs, gflow, taps, source, lmbda, owner=latents)

    searches = [search() for _ in range(1 + runs)][1:]
    one = searches[0]
    steps = [[writer.q_step_range(g)[0] for g in range(8)] for _ in range(2)]
    res["modules"] = {}
    for k, t in enumerate(one.tables):
        secs = [s.pricing[k].seconds for s in searches]
        build = [s.pricing[k].build_seconds for s in searches]
        _, gw, gb = next(m for m in MODULES if m[0] == t.module)
        partner = build_network(archs[1 - t.role], floats[1 - t.role], steps[1 - t.role])
        pairs = []
        for c in t.cells:
            if c.feasible:
                s = list(steps[t.role])
                s[gw], s[gb] = c.q_w, c.q_b
                net = build_network(archs[t.role], floats[t.role], s)
                pairs.append((net, partner) if t.role == 0 else (partner, net))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a, b in pairs:  # the yardstick: one candidate at a time through the calls the parent commit has
            with InterRdEvaluator(0) as ev:
                ev.add(frame_type, (a.header, a.bytes_nn, ptrs[0]), (b.header, b.bytes_nn, ptrs[1]), refs, gflow, taps, source, owner=latents)
                ev.evaluate(lmbda)
        alone = time.perf_counter() - t0
        res["modules"][f"{ROLES[t.role]} {t.module}"] = {
            "candidates": len(t.cells), "feasible": len(pairs), "per_launch": one.pricing[k].chunk,
            "sweep_s": {"median": round(statistics.median(secs), 4), "min": round(min(secs), 4), "max": round(max(secs), 4)},
            "of_which_building_candidates_s": round(statistics.median(build), 4),
            "one_at_a_time_s": round(alone, 4), "ratio": round(alone / statistics.median(secs), 2)}
        if t.chosen is not None:
            steps[t.role][gw], steps[t.role][gb] = t.cells[t.chosen].q_w, t.cells[t.chosen].q_b
    with InterRdEvaluator(0) as ev:
        ev.add(frame_type, (archs[0], ccs[0][1], ptrs[0]), (archs[1], ccs[1][1], ptrs[1]), refs, gflow, taps, source, owner=latents)
        c = ev.evaluate(lmbda)[0]
    res["reached"] = {"stream": {"cost": c.cost, "bytes_nn": len(ccs[0][1]) + len(ccs[1][1]), "psnr_db": round(c.quality.psnr_db, 4), "bits": round(c.bits, 1)},
                      "searched": {"cost": one.candidate.cost, "bytes_nn": sum(len(n.bytes_nn) for n in one.roles),
                                   "psnr_db": round(one.candidate.quality.psnr_db, 4), "bits": round(one.candidate.bits, 1)},
                      "steps": [list(n.header.nn_q_step_log2) for n in one.roles]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--no-replaced", action="store_true", help="skip the replaced route (profiling runs)")
    ap.add_argument("--ddeltas", action="store_true", help="time the distortion deltas instead")
    ap.add_argument("--probe-slots", type=int, default=16)
    ap.add_argument("--rdoq", action="store_true", help="time one requantisation step and the evaluation that feeds it instead")
    ap.add_argument("--lmbda", type=float, default=1e-3)
    ap.add_argument("--sets", default="kodim14,kodak24", help="with --rdoq: which of the two sets to measure")
    ap.add_argument("--inter", action="store_true", help="time the distortion deltas of P / B frames instead")
    ap.add_argument("--inter-sets", default="vid5,1080p", help="with --inter: which of the two sets to measure")
    ap.add_argument("--joint", action="store_true", help="with --inter: the descent of the frames, alternating and joint, instead")
    ap.add_argument("--rounds", type=int, default=8, help="with --inter --joint: rounds of selection per step")
    ap.add_argument("--grids", default="0,1,2", help="with --inter --joint: the grids that may move, in both cool-chics")
    ap.add_argument("--max-steps", type=int, default=400, help="with --inter --joint: steps of a descent at most")
    ap.add_argument("--dependents", action="store_true", help="time the distortion deltas through the direct dependents of an I frame instead")
    ap.add_argument("--follow", action="store_true", help="time an RDOQ step of an I frame whose claims follow the flows into its dependents instead")
    ap.add_argument("--networks", action="store_true", help="time the search over the networks' quantisation steps instead")
    ap.add_argument("--network-sets", default="kodak,1080p", help="with --networks: which of the two frames to measure")
    ap.add_argument("--arm-refine", action="store_true", help="time the ARM parameter table and one descent instead")
    ap.add_argument("--ifce-refine", action="store_true", help="time the IFCE parameter table and the ARM + IFCE descent instead")
    ap.add_argument("--refine-sets", default="kodim14,kodak24,1080p", help="with --arm-refine / --ifce-refine: which of the three inputs to measure")
    a = ap.parse_args()
    if a.arm_refine or a.ifce_refine:
        from cool_chic_amd.bitstream.decode import _split_frame
        from cool_chic_amd.bitstream.header import VideoHeader

        line = {"tool": "rd_bench --ifce-refine" if a.ifce_refine else "rd_bench --arm-refine"}
        k24 = synth.workload("kodak24")["streams"]
        if "kodim14" in a.refine_sets.split(","):
            line["kodim14"] = measure_arm_table([synth.split_image_stream(k24[0])], a.runs, 3, 25, ifce=a.ifce_refine)
        if "kodak24" in a.refine_sets.split(","):
            line["kodak24"] = measure_arm_table([synth.split_image_stream(bs) for bs in k24], a.runs, 3, 0, ifce=a.ifce_refine)
        if "1080p" in a.refine_sets.split(","):
            fh, ccs, _ = _split_frame(VideoHeader().read_header(synth.gop1080p(2)[0]))
            assert fh.get_value("frame_type") == "I"
            line["gop1080p_I"] = measure_arm_table([(ccs[0][0].raw, ccs[0][1], ccs[0][2])], a.runs, 3, 0, ifce=a.ifce_refine)
        print(json.dumps(line))
        return
    if a.networks and a.inter:
        runs = min(a.runs, 5)
        line = {"tool": "rd_bench --networks --inter", "runs": runs}
        if "vid5" in a.inter_sets.split(","):
            line["vid5_P"] = measure_inter_networks(synth._golden("vid5")[0], 1, runs, a.lmbda)
        if "1080p" in a.inter_sets.split(","):
            line["1080p_P"] = measure_inter_networks(ip_1080p(), 1, runs, a.lmbda)
            line["gop1080p_B"] = measure_inter_networks(synth.gop1080p(2)[0], 2, runs, a.lmbda)
        print(json.dumps(line))
        return
    if a.networks and a.dependents:
        runs = min(a.runs, 5)
        line = {"tool": "rd_bench --networks --dependents", "runs": runs}
        if "vid5" in a.inter_sets.split(","):
            line["vid5_I"] = measure_network_dependents(synth._golden("vid5")[0], runs, [1e-3, 1e-2])
        if "1080p" in a.inter_sets.split(","):
            line["gop1080p33_I"] = measure_network_dependents(synth.gop1080p(32)[0], runs, [1e-3, 1e-2])
        print(json.dumps(line))
        return
    if a.networks:
        from cool_chic_amd.bitstream.decode import _split_frame
        from cool_chic_amd.bitstream.header import VideoHeader

        runs = min(a.runs, 5)
        line = {"tool": "rd_bench --networks", "runs": runs}
        if "kodak" in a.network_sets.split(","):
            line["kodak_512x768"] = measure_networks(*synth.split_image_stream(synth.workload("kodak24")["streams"][0]), 8, 0, runs, [1e-3, 1e-4, 1e-2], 8)
        if "1080p" in a.network_sets.split(","):
            rest = VideoHeader().read_header(synth.gop1080p(2)[0])
            fh, ccs, rest = _split_frame(rest)
            assert fh.get_value("frame_type") == "I"
            fdt = ["rgb", "yuv420", "yuv444"].index(fh.get_value("frame_data_type"))
            line["gop1080p_I"] = measure_networks(ccs[0][0].raw, ccs[0][1], ccs[0][2], fh.get_value("bitdepth"), fdt, runs, [1e-3], 0)
        print(json.dumps(line))
        return
    if a.follow:
        line = {"tool": "rd_bench --follow", "runs": a.runs}
        args = (a.runs, a.lmbda, a.rounds, [int(g) for g in a.grids.split(",") if g != ""], a.probe_slots)
        if "vid5" in a.inter_sets.split(","):
            line["vid5_I"] = measure_follow(synth._golden("vid5")[0], *args)
        if "1080p" in a.inter_sets.split(","):
            line["gop1080p_I"] = measure_follow(synth.gop1080p(2)[0], *args)
        print(json.dumps(line))
        return
    if a.dependents:
        runs = min(a.runs, 5)
        line = {"tool": "rd_bench --dependents", "runs": runs}
        if "vid5" in a.inter_sets.split(","):
            line["vid5_I"] = measure_dependents(synth._golden("vid5")[0], runs, a.probe_slots)
        if "1080p" in a.inter_sets.split(","):
            line["gop1080p_I"] = measure_dependents(synth.gop1080p(2)[0], runs, a.probe_slots)
        print(json.dumps(line))
        return
    if a.inter and a.joint:
        line = {"tool": "rd_bench --inter --joint", "runs": a.runs}
        args = (a.runs, a.lmbda, a.rounds, [int(g) for g in a.grids.split(",") if g != ""], a.max_steps)
        if "vid5" in a.inter_sets.split(","):
            vid5 = synth._golden("vid5")[0]
            line["vid5_P"] = measure_inter_descent(vid5, 1, *args)
            line["vid5_B"] = measure_inter_descent(vid5, 3, *args)
        if "1080p" in a.inter_sets.split(","):
            line["gop1080p_B"] = measure_inter_descent(synth.gop1080p(2)[0], 2, *args)
        print(json.dumps(line))
        return
    if a.inter:
        line = {"tool": "rd_bench --inter", "runs": a.runs}
        if "vid5" in a.inter_sets.split(","):
            vid5 = synth._golden("vid5")[0]
            line["vid5_P"] = measure_inter(vid5, 1, a.runs, a.probe_slots)
            line["vid5_B"] = measure_inter(vid5, 3, a.runs, a.probe_slots)
        if "1080p" in a.inter_sets.split(","):
            line["gop1080p_B"] = measure_inter(synth.gop1080p(2)[0], 2, a.runs, a.probe_slots)
        print(json.dumps(line))
        return
    k24 = synth.workload("kodak24")["streams"]
    if a.rdoq:
        line = {"tool": "rd_bench --rdoq", "runs": a.runs}
        if "kodim14" in a.sets.split(","):
            line["kodim14"] = measure_rdoq(k24[:1], a.runs, a.lmbda, True)
        if "kodak24" in a.sets.split(","):
            line["kodak24"] = measure_rdoq(k24, a.runs, a.lmbda, False)
        print(json.dumps(line))
        return
    if a.ddeltas:
        print(json.dumps({"tool": "rd_bench --ddeltas", "runs": a.runs, "kodim14": measure_ddeltas(k24[:1], a.runs, a.probe_slots),
                          "kodak24": measure_ddeltas(k24, a.runs, a.probe_slots)}))
        return
    print(json.dumps({"tool": "rd_bench", "runs": a.runs, "kodim14": measure(k24[:1], a.runs, not a.no_replaced),
                      "kodak24": measure(k24, a.runs, not a.no_replaced)}))


if __name__ == "__main__":
    main()
