"""Helpers of tests/test_stream_contract.py: the gate, the gated call and the case table (no tests here).

include/ccd.h promises for nearly every entry point with a `void* stream` that the call only enqueues on that stream, reads its
device inputs in stream order, that work enqueued on the stream afterwards sees its results, and that the handle's destroy drains
the streams it was given.  A CASE names one entry point with its smallest input; the harness runs it on a side stream behind a
bounded delay (torch.cuda._sleep, an ordinary kernel that ends by itself) while the tensors the handle was added with still hold
POISON - another valid input of the same shape and type.  The real input is copied in on the side stream behind the delay, so a
launch or an upload that lands on another stream, a missing join or a result read too early gives the poison's result, which
every case first shows to differ from the expected one.

The expected results are those of the same job on the default stream with torch.cuda.synchronize() on both sides, compared bit
for bit (floats through their bytes); the one exception is compute_rate's total, whose atomic adds have no fixed order and which
keeps tests/test_rate_model.py's _sum_bound."""
import ctypes as C
import dataclasses
import math
import re
import struct
import time
from typing import NamedTuple

import numpy as np

MIN_DELAY_MS, MAX_DELAY_MS, HOST_FACTOR, ATTEMPTS = 20.0, 500.0, 20.0, 3


# ---- what is covered (read by the CPU coverage test; no device needed) -------------------------------------------------------------
# entry point of include/ccd.h with a `void* stream` -> the cases of CASES that call it
COVERAGE = {
    "ccd_compute_rate": ["rate", "rate_total"],
    "ccd_quality_score_batch": ["quality_decoded", "quality_sources"],
    "ccd_quality_finish_batch": ["quality_decoded", "quality_sources"],
    "ccd_png_pack": ["png_level0", "png_level1"],
    "ccd_png_finish": ["png_level0", "png_level1"],
    "ccd_png_pack_batch": ["png_batch_level0", "png_batch_level1"],
    "ccd_png_finish_batch": ["png_batch_level0", "png_batch_level1"],
    "ccd_enc_run": ["enc_run"],
    "ccd_enc_wait": ["enc_run", "enc_measure", "enc_measure_deltas", "enc_param_deltas", "enc_ifce_deltas"],
    "ccd_enc_measure": ["enc_measure"],
    "ccd_enc_measure_deltas": ["enc_measure_deltas"],
    "ccd_enc_measure_param_deltas": ["enc_param_deltas"],
    "ccd_enc_measure_ifce_deltas": ["enc_ifce_deltas"],
    "ccd_batch_copy_planes_async": ["decode_given"],
    "ccd_dsens_run": ["dsens_intra_dependent", "dsens_inter_p_residue", "dsens_inter_p_motion", "dsens_inter_b_residue"],
    "ccd_dsens_wait": ["dsens_intra_dependent", "dsens_inter_p_residue", "dsens_inter_p_motion", "dsens_inter_b_residue"],
    "ccd_rdoq_step": ["rdoq_rounds1"],
    "ccd_rdoq_step_rounds": ["rdoq_rounds8", "rdoq_follow"],
    "ccd_rdoq_wait": ["rdoq_rounds1", "rdoq_rounds8", "rdoq_follow"],
    "ccd_iscore_run": ["iscore_residue", "iscore_motion", "iscore_references", "iscore_sources"],
    "ccd_iscore_wait": ["iscore_residue", "iscore_motion", "iscore_references", "iscore_sources"],
    "ccd_inter_reconstruct": ["reconstruct_p", "reconstruct_b"],
}
# ccd_batch_add_latents takes no stream of its own: its device latents are read by ccd_batch_run, which "decode_given" gates
EXEMPT = {
    "ccd_batch_prepare": "tests/test_gpu_parity.py: prepare / run on two streams, a run behind a stream wait",
    "ccd_batch_run": "tests/test_gpu_parity.py (coded slots); the given-latent path runs here as decode_given",
    "ccd_batch_run_stage": "tests/test_gpu_parity.py: the stages one by one",
    "ccd_batch_wait": "tests/test_gpu_parity.py; every case of decode_given ends in it",
    "ccd_batch_copy_latent": "synchronous on its stream: returns with the copy done",
    "ccd_batch_copy_plane": "synchronous on its stream: returns with the copy done",
    "ccd_batch_copy_output": "synchronous on its stream: returns with the copy done",
    "ccd_batch_copy_dense": "synchronous on its stream: returns with the copy done",
    "ccd_decode_coolchic": "one-shot decode that owns its batch; synchronous for a host output (tests/test_gpu_parity.py)",
}


def stream_entry_points(header_text):
    """Every function of the header that has a `void* stream` parameter."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    names = []
    for m in re.finditer(r"\b(ccd_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            names.append(m.group(1))
    return names


# ---- canonical form of a result: equal canonical forms <=> equal bits --------------------------------------------------------------
def canon(obj):
    """Results as nested tuples of ints, strings and bytes: floats and arrays through their bytes, so that NaN equals NaN and
    -0.0 differs from 0.0."""
    import torch

    if isinstance(obj, torch.Tensor):
        return canon(obj.detach().cpu().contiguous().view(torch.uint8).numpy()) + (str(obj.dtype), tuple(obj.shape))
    if isinstance(obj, np.ndarray):
        return ("array", str(obj.dtype), obj.shape, np.ascontiguousarray(obj).tobytes())
    if isinstance(obj, (bool, int, np.integer)):
        return int(obj)
    if isinstance(obj, (float, np.floating)):
        return ("f64", struct.pack("<d", float(obj)))
    if isinstance(obj, (bytes, str)) or obj is None:
        return obj
    if dataclasses.is_dataclass(obj):
        return tuple((f.name, canon(getattr(obj, f.name))) for f in dataclasses.fields(obj))
    if isinstance(obj, C.Structure) or isinstance(obj, C.Array):
        return bytes(obj)
    if isinstance(obj, dict):
        return tuple((k, canon(v)) for k, v in sorted(obj.items()))
    if isinstance(obj, (tuple, list)):
        return tuple(canon(v) for v in obj)
    raise TypeError(f"no canonical form for {type(obj).__name__}")


# ---- the gate ----------------------------------------------------------------------------------------------------------------------
class Gate:
    """A side stream with a bounded delay in front of it, and a second, idle stream."""

    def __init__(self):
        import torch

        self.side = torch.cuda.Stream(device="cuda:0")
        self.other = torch.cuda.Stream(device="cuda:0")
        torch.cuda._sleep(1_000_000)  # the first launch of the spin kernel is not timed
        torch.cuda.synchronize()
        n = 10_000_000
        t0 = time.perf_counter()
        torch.cuda._sleep(n)
        torch.cuda.synchronize()
        self.cycles_per_ms = n / ((time.perf_counter() - t0) * 1e3)
        self.host_ms, self.delay_ms = [], []  # every gated call's host time and delay, for the ranges the log ends with
        print(f"gate: {self.cycles_per_ms:.0f} spin cycles per millisecond")

    def arm(self, delay_ms):
        """Puts the delay on the side stream; returns the event `delay_done` recorded behind it."""
        import torch

        assert 0 < delay_ms <= MAX_DELAY_MS
        done = torch.cuda.Event()
        with torch.cuda.stream(self.side):
            torch.cuda._sleep(int(delay_ms * self.cycles_per_ms))
            done.record(self.side)
        return done


class Gated(NamedTuple):
    live: object     # the tensor the handle was added with
    real: object     # staging: the input of the expected result
    poison: object   # staging: another valid input


def first_delay(host_ms):
    return min(MAX_DELAY_MS, max(MIN_DELAY_MS, HOST_FACTOR * host_ms))


class Case:
    """One entry point with its smallest input.  A subclass builds its fixed inputs and `self.gated` in __init__, and says how to
    open a handle over the live tensors, enqueue the entry point, wait, and read the results."""

    name = ""
    enqueues = True        # the header says the call only enqueues (P2); False: it may synchronise, and is then conclusive as it is
    foreign_wait = False   # the handle's wait takes a stream of its own
    has_handle = True      # there is a destroy (P4)

    def open(self):
        return None

    def call(self, h, stream):
        raise NotImplementedError

    def wait(self, h, stream):
        raise NotImplementedError

    def read(self, h):
        raise NotImplementedError

    def early(self, h):
        """Device tensors whose address the caller may hold before the wait (P3)."""
        return []

    def early_result(self, snaps, result):
        """What the snapshots of early() must equal, in the terms of read()'s result."""
        return canon(snaps)

    def same(self, got, want):
        return canon(got) == canon(want)

    def same_early(self, got, want):
        return canon(got) == canon(want)

    def close(self, h):
        if h is not None:
            h.close()

    def fill(self, which):
        """The live tensors hold the real input or the poison; device idle on return."""
        import torch

        for g in self.gated:
            g.live.copy_(getattr(g, which))
        torch.cuda.synchronize()


def stream_sync(stream):
    """Waits for a raw hipStream_t (0: the default stream) through torch."""
    import torch

    if stream:
        torch.cuda.ExternalStream(stream, device="cuda:0").synchronize()
    else:
        torch.cuda.default_stream(0).synchronize()


class Reference(NamedTuple):
    want: object
    poison: object
    want_early: object


_REFERENCES = {}


def reference(case):
    """(expected result, the poison's result, expected early tensors) from a handle of its own on the default stream with
    torch.cuda.synchronize() on both sides; computed once per case.  Fails when the poison cannot be told from the real input."""
    import torch

    if case.name not in _REFERENCES:
        h = case.open()
        try:
            out = []
            for which in ("poison", "real"):
                case.fill(which)
                case.call(h, 0)
                case.wait(h, 0)
                torch.cuda.synchronize()
                res = case.read(h)
                out.append((res, case.early_result([t.clone() for t in case.early(h)], res)))
                torch.cuda.synchronize()
        finally:
            case.close(h)
        (poison, _), (want, want_early) = out
        assert not case.same(poison, want) and not case.same(want, poison), f"{case.name}: the poison gives the expected result"
        _REFERENCES[case.name] = Reference(want, poison, want_early)
    return _REFERENCES[case.name]


def warm_up(case, h):
    """One run with the poison on the default stream: planning and pool growth are behind it, stale memory holds the poison's
    result, and the call's host time sizes the delay.  Returns that time in ms."""
    import torch

    case.fill("poison")
    t0 = time.perf_counter()
    case.call(h, 0)
    host_ms = (time.perf_counter() - t0) * 1e3
    case.wait(h, 0)
    torch.cuda.synchronize()
    return host_ms


class Outcome(NamedTuple):
    got: object            # read() after the wait (None after a destroy)
    snaps: object          # early_result of the snapshots (None unless asked for)
    after_call: bool       # delay_done.query() when the call returned
    after_snapshot: bool   # ... when the snapshot copies were enqueued
    before_close: bool
    after_close: bool
    host_ms: float
    delay_ms: float


def gated_call(case, gate, h, delay_ms, call_on=None, wait_on=None, snapshot=False, destroy=False):
    """One gated call: the delay on the side stream and `delay_done` behind it, the real inputs copied over the poison on the side
    stream, the entry point on `call_on` (the side stream) with no host synchronisation before it; then snapshot copies on the
    side stream, and the wait on `wait_on` (the side stream) or the destroy."""
    import torch

    side = gate.side
    call_on = side if call_on is None else call_on
    wait_on = call_on if wait_on is None else wait_on
    case.fill("poison")
    early = case.early(h) if snapshot else []
    snaps = [torch.empty_like(t) for t in early]
    torch.cuda.synchronize()
    done = gate.arm(delay_ms)
    with torch.cuda.stream(side):
        for g in case.gated:
            g.live.copy_(g.real, non_blocking=True)
    t0 = time.perf_counter()
    case.call(h, call_on.cuda_stream)
    host_ms = (time.perf_counter() - t0) * 1e3
    after_call = done.query()
    after_snapshot = after_call
    if snapshot:
        with torch.cuda.stream(side):
            for s, t in zip(snaps, early):
                s.copy_(t, non_blocking=True)
        after_snapshot = done.query()
    got = snap_result = None
    before_close = after_close = False
    if destroy:
        before_close = done.query()
        case.close(h)
        after_close = done.query()
    else:
        if call_on is not side:  # the sensitivity test: the idle stream ends while the delay still runs
            call_on.synchronize()
            after_call = done.query()
        case.wait(h, wait_on.cuda_stream)
        got = case.read(h)
    side.synchronize()
    torch.cuda.synchronize()
    if snapshot:
        snap_result = case.early_result(snaps, got)
    gate.host_ms.append(host_ms)
    gate.delay_ms.append(delay_ms)
    return Outcome(got, snap_result, after_call, after_snapshot, before_close, after_close, host_ms, delay_ms)


def conclusive_call(case, gate, make_handle, warm_ms, what, is_conclusive, check, **kw):
    """Repeats a gated call with the delay doubled while it is inconclusive - a measurement repeated, never a mismatch: `check`
    runs on every attempt, so a wrong result fails at once - at most ATTEMPTS times.  Returns the conclusive Outcome."""
    delay = first_delay(warm_ms)
    log = []
    for _ in range(ATTEMPTS):
        o = gated_call(case, gate, make_handle(), delay, **kw)
        ok = bool(is_conclusive(o))
        log.append(f"host {o.host_ms:.3f} ms, delay {o.delay_ms:.1f} ms")
        print(f"{case.name} [{what}]: warm-up call {warm_ms:.3f} ms, gated call {o.host_ms:.3f} ms on the host, delay {o.delay_ms:.1f} ms: "
              f"{'conclusive' if ok else 'inconclusive'}")
        check(o)
        if ok:
            return o
        delay = min(MAX_DELAY_MS, 2.0 * delay)
    raise AssertionError(f"{case.name} [{what}]: inconclusive {ATTEMPTS} times - the delay had ended where it must still run ({'; '.join(log)})")


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _planes_dev(planes, bitdepth):
    """Integer planes of any integer dtype as contiguous device tensors of the library's sample type."""
    import torch

    dt = torch.uint8 if bitdepth == 8 else torch.uint16
    return [torch.from_numpy(np.asarray(p).astype(np.int32)).cuda().to(dt).contiguous() for p in planes]


def _gate_all(reals, poisons):
    """Gated triples of two equal-shaped lists of device tensors: the live tensors start as clones of the poison."""
    return [Gated(p.clone(), r, p) for r, p in zip(reals, poisons)]


class RateCase(Case):
    """ccd_compute_rate over tests/test_rate_model.py's base tensors (family A, seeded), 4097 symbols so that the tail kernel runs
    behind the vector kernel; the poison is another seeded draw of the same family."""

    has_handle = False
    N = 4097

    def __init__(self, total):
        import torch

        import rate_model_ref as R

        self.name = "rate_total" if total else "rate"
        self.total = total
        x, mu, scale, _, _ = R.family("A")
        draws = []
        for seed in (5, 6):
            idx = torch.randperm(x.numel(), generator=torch.Generator().manual_seed(seed))[:self.N]
            draws.append([t[idx].cuda() for t in (x, mu, scale)])
        self.gated = _gate_all(*draws)
        self.rate = torch.zeros(self.N, dtype=torch.float32, device="cuda")
        self.sum = torch.zeros(1, dtype=torch.float64, device="cuda")

    def call(self, h, stream):
        from cool_chic_amd._lib import check, lib

        x, mu, scale = (g.live.data_ptr() for g in self.gated)
        check(lib().ccd_compute_rate(0, C.c_void_p(stream or None), C.c_void_p(x), C.c_void_p(mu), C.c_void_p(scale), self.N,
                                     C.c_void_p(self.rate.data_ptr()), C.c_void_p(self.sum.data_ptr()) if self.total else None),
              "ccd_compute_rate")

    def wait(self, h, stream):
        stream_sync(stream)

    def read(self, h):
        return (self.rate.clone(), float(self.sum.item()) if self.total else 0.0)

    def early(self, h):
        return [self.rate, self.sum] if self.total else [self.rate]

    def early_result(self, snaps, result):
        return (snaps[0].clone(), float(snaps[1].item()) if self.total else 0.0)

    def same(self, got, want):
        """The rates bit for bit; the total within test_rate_model.py's _sum_bound of the exact sum of the expected rates."""
        if canon(got[0]) != canon(want[0]):
            return False
        if not self.total:
            return True
        s = math.fsum(want[0].double().cpu().tolist())
        return abs(got[1] - s) <= self.N * 2.0 ** -53 * s

    same_early = same


class QualityCase(Case):
    """One 177 x 200 16-bit RGB frame (176 is the MS-SSIM floor) and one 38 x 100 4:2:0 8-bit frame, which is below the floor and
    so scored for its squared error only, in one batch.  `which`: the decoded planes are gated and the sources fixed, or the other
    way round."""

    foreign_wait = True

    def __init__(self, which):
        import quality_ref as Q

        self.name = f"quality_{which}"
        shapes = [(16, [(177, 200)] * 3), (8, [(38, 100), (19, 50), (19, 50)])]
        self.bitdepths = [bd for bd, _ in shapes]

        def pictures(seed):
            src = [[Q.textured(seed + 10 * f + p, h, w, bd) for p, (h, w) in enumerate(hw)] for f, (bd, hw) in enumerate(shapes)]
            dec = [[Q.with_noise(s, seed + 500 + 10 * f + p, bd, Q.LIGHT) for p, s in enumerate(frame)]
                   for f, (frame, (bd, _)) in enumerate(zip(src, shapes))]
            return ([_planes_dev(f, bd) for f, bd in zip(dec, self.bitdepths)], [_planes_dev(f, bd) for f, bd in zip(src, self.bitdepths)])

        (dec, src), (dec2, src2) = pictures(100), pictures(200)
        flat = lambda frames: [p for f in frames for p in f]  # noqa: E731
        if which == "decoded":
            self.gated = _gate_all(flat(dec), flat(dec2))
            live = [g.live for g in self.gated]
            self.decoded, self.sources = [live[:3], live[3:]], src
        else:
            self.gated = _gate_all(flat(src), flat(src2))
            live = [g.live for g in self.gated]
            self.decoded, self.sources = dec, [live[:3], live[3:]]

    def open(self):
        from cool_chic_amd.quality import QualityMeter

        return QualityMeter(0)

    def call(self, h, stream):
        h.score_planes_async(self.decoded, self.sources, self.bitdepths, True, stream=stream)

    def wait(self, h, stream):
        from cool_chic_amd._lib import QualityResult, check, lib

        self._res = (QualityResult * 2)()
        check(lib().ccd_quality_finish_batch(h._h, C.c_void_p(stream or None), self._res, 2), "ccd_quality_finish_batch")

    def read(self, h):
        assert [int(self._res[0].n_scales[p]) for p in range(3)] == [5, 5, 5] and not any(self._res[1].n_scales)
        return bytes(self._res)


class PngCase(Case):
    """A 40 x 50 `photo` picture of tests/png_pictures.py at level 0 or 1, alone (pack / finish) or as a batch of two (pack_batch /
    finish_batch); the poison is the photo of another seed.  The `out` buffers are the early tensors."""

    foreign_wait = True

    def __init__(self, level, batch):
        import torch

        import png_pictures as P
        from cool_chic_amd.io.png import PngPacker

        self.name = f"png_{'batch_' if batch else ''}level{level}"
        self.level, self.n = level, 2 if batch else 1
        self.batch = batch
        h, w = 40, 50
        real = [_dev(P._pictures(h, w, seed)["photo"]) for seed in range(self.n)]
        poison = [_dev(P._pictures(h, w, seed)["photo"]) for seed in range(10, 10 + self.n)]
        self.gated = _gate_all(real, poison)
        self.h, self.w = h, w
        self.out = [torch.zeros(PngPacker.bound(h, w) + 4, dtype=torch.uint8, device="cuda") for _ in range(self.n)]

    def open(self):
        from cool_chic_amd.io.png import PngPacker

        return PngPacker(0, self.level)

    def _items(self):
        step = self.h * self.w
        return [(g.live.data_ptr(), g.live.data_ptr() + step, g.live.data_ptr() + 2 * step, self.h, self.w, o) for g, o in zip(self.gated, self.out)]

    def call(self, h, stream):
        if self.batch:
            h.pack_batch_async(self._items(), stream)
        else:
            r, g, b, hh, ww, out = self._items()[0]
            h.pack_async(r, g, b, hh, ww, out, stream)

    def wait(self, h, stream):
        self._sizes = h.finish_batch(stream) if self.batch else [h.finish(stream)]

    def read(self, h):
        return [o[:n].cpu().numpy().tobytes() for o, n in zip(self.out, self._sizes)]

    def early(self, h):
        return self.out

    def early_result(self, snaps, result):
        """The bytes of the file: what lies behind finish's size in `out` is scratch."""
        return canon([s[:len(r)].cpu().numpy().tobytes() for s, r in zip(snaps, result)])


class _Rgb192:
    """rgb192's cool-chic with two latent sets inside [-64, 63]: the fixture's own latents with a seeded tenth of the positions
    moved by +-1 (tests/test_rdoq.py's _Picture), seeds 0 and 1, each in one device buffer with 256-byte aligned grids."""

    def __init__(self, oracle):
        from test_rdoq import _Picture, _picture

        self.pic = _picture(oracle, "rgb192")
        self.geo = self.pic.geo
        self.real = self.pic.device_latents()
        self.poison = _Picture(oracle, "rgb192", seed=1).device_latents()
        assert not bool((self.real == self.poison).all())

    def gated(self):
        return [Gated(self.poison.clone(), self.real, self.poison)]


class EncCase(Case):
    """EncodeBatch over rgb192 added with add_device: the latents are the gated tensor."""

    foreign_wait = True
    KINDS = ("run", "measure", "measure_deltas", "param_deltas", "ifce_deltas")

    def __init__(self, rgb, kind):
        self.name = f"enc_{kind}"
        self.kind, self.rgb = kind, rgb
        self.gated = rgb.gated()

    def open(self):
        from cool_chic_amd import EncodeBatch

        enc = EncodeBatch(0)
        live, geo = self.gated[0].live, self.rgb.geo
        enc.add_device(geo.arch, geo.nn, self.rgb.pic.ptrs(live), owner=live)
        return enc

    def call(self, h, stream):
        {"run": h.run, "measure": lambda s: h.measure(s, rate_map=True), "measure_deltas": h.measure_deltas,
         "param_deltas": h.measure_param_deltas, "ifce_deltas": h.measure_ifce_deltas}[self.kind](stream)

    def wait(self, h, stream):
        h.wait(stream)

    def read(self, h):
        import torch

        n = self.rgb.geo.n
        if self.kind == "run":
            return (h.bytes(0), h.slot_status(0))
        rate = tuple(h.rate(0))
        if self.kind == "measure":
            return (rate, [torch.as_tensor(h.rate_map(0, g), device="cuda").clone() for g in range(n)])
        if self.kind == "measure_deltas":
            return (rate, [torch.as_tensor(h.delta_map(0, g), device="cuda").clone() for g in range(n)])
        return (rate, tuple(h.param_deltas(0) if self.kind == "param_deltas" else h.ifce_deltas(0)))


class DecodeCase(Case):
    """DecodeBatch.add_latents_device + run over rgb192, followed on the same stream by the writer's copy of the planes into
    pinned memory (ccd_batch_copy_planes_async).  The planes, the float output and the ingested latents are the early tensors."""

    foreign_wait = True

    def __init__(self, rgb):
        self.name = "decode_given"
        self.rgb = rgb
        self.gated = rgb.gated()

    def open(self):
        import torch

        from cool_chic_amd import DecodeBatch

        b = DecodeBatch(0)
        live, geo = self.gated[0].live, self.rgb.geo
        b.add_latents_device(geo.arch, geo.nn, self.rgb.pic.ptrs(live), geo.bd, geo.fdt, owner=live)
        total, b._layout = b.planes_layout()
        b._pinned = torch.zeros(total, dtype=torch.uint8, pin_memory=True)
        return b

    def call(self, h, stream):
        h.run(stream)
        h.copy_planes_async(h._pinned.data_ptr(), h._layout, stream)

    def wait(self, h, stream):
        h.wait(stream)

    def read(self, h):
        views = h.plane_views(h._pinned.numpy(), h._layout)
        return ([p.copy() for p in views[0]], h.planes(0), h.output(0), [h.latent(0, g) for g in range(self.rgb.geo.n)])

    def early(self, h):
        import torch

        from cool_chic_amd._handle import _DevArray

        geo = self.rgb.geo
        lat = [_DevArray(p, geo.hw[g], "|i1", h) for g, p in enumerate(h.latent_ptrs(0))]
        return [torch.as_tensor(a, device="cuda") for a in [h.plane_device(0, p) for p in range(3)] + [h.output_device(0)] + lat]

    def early_result(self, snaps, result):
        return canon([s.cpu().numpy() for s in snaps])


class DsensCase(Case):
    """DistortionDeltas.run.  "intra_dependent": the intra frame of vid3_ldp with the P frame that predicts from it
    (tests/dependent_cases.py's smallest pair): the candidate's latents and the dependent's two float outputs are gated.
    "inter_*": one cool-chic of a P frame (vid3_ldp frame 1) or of a B frame of vid5: its latents and the partner's output."""

    foreign_wait = True

    def __init__(self, kind):
        import dependent_cases as dc
        import inter_cases as ic

        self.name = f"dsens_{kind}"
        self.kind = kind
        if kind == "intra_dependent":
            self.ref = dc.intra("vid3_ldp")
            f = ic.case("vid3_ldp", 1)
            cc = self.ref.cc
            self.lat = Gated(_dev(cc.flat(cc.lat2)), cc.lat_dev, _dev(cc.flat(cc.lat2)))
            self.res = Gated(f.out2["residue"].clone(), f.out["residue"], f.out2["residue"])
            self.mot = Gated(f.out2["motion"].clone(), f.out["motion"], f.out2["motion"])
            self.dep = dc.Dependent(f, 0)
            self.dep.residue = self.res.live
            self.gated = [self.lat, self.res, self.mot]
            self.n = self.ref.n
        else:
            _, frame, self.role = kind.split("_")
            self.case = f = ic.case("vid3_ldp", 1) if frame == "p" else ic.case("vid5", self._b_frame("vid5"))
            assert f.frame_type == (1 if frame == "p" else 2)
            cc = f.cc[self.role]
            other = ic.ROLES[1 - ic.ROLES.index(self.role)]
            self.lat = Gated(_dev(cc.flat(cc.lat2)), cc.lat_dev, _dev(cc.flat(cc.lat2)))
            self.partner = Gated(f.out2[other].clone(), f.out[other], f.out2[other])
            self.gated = [self.lat, self.partner]
            self.n = cc.n

    @staticmethod
    def _b_frame(name):
        import inter_cases as ic

        return next(k for k, (fh, *_) in enumerate(ic.parse_video(name)) if fh.frame_type == 2)

    def open(self):
        from cool_chic_amd import DistortionDeltas

        d = DistortionDeltas(0, 16)
        if self.kind == "intra_dependent":
            slot = self.ref.add_to(d, lat_dev=self.lat.live)
            self.dep.add_to(d, slot, motion=self.mot.live)
        else:
            self.case.add_to(d, self.role, lat_dev=self.lat.live, partner=self.partner.live)
        return d

    def call(self, h, stream):
        h.run(stream)

    def wait(self, h, stream):
        h.wait(stream)

    def read(self, h):
        import torch

        own = [torch.as_tensor(h.delta_map(0, g), device="cuda").clone() for g in range(self.n)]
        if self.kind != "intra_dependent":
            return (own,)
        return (own, [torch.as_tensor(h.dep_delta_map(0, g), device="cuda").clone() for g in range(self.n)],
                [h.dep_conflicts(0, g) for g in range(self.n)])


class RdoqCase(Case):
    """RdoqStep.step over tests/test_rdoq.py's crafted maps (odd18x65, seed 1): the two delta maps of every grid are gated, the
    poison is all-zero maps, which offer no move.  rounds 1 goes through ccd_rdoq_step, 8 through ccd_rdoq_step_rounds; "follow":
    a second slot is the residue of a P frame that predicts from the first, whose claims follow seeded flows into it.  The
    latents, which a step moves in place, are put back before every run and are the early tensor."""

    foreign_wait = True

    def __init__(self, kind):
        import torch

        from test_rdoq import _Synth

        self.name = f"rdoq_{kind}"
        self.kind = kind
        self.rounds = 1 if kind == "rounds1" else 8
        self.syns = [_Synth("odd18x65", 1).upload() for _ in range(2 if kind == "follow" else 1)]
        self.gated = []
        for s in self.syns:
            start = s.buf.clone()
            self.gated.append(Gated(s.buf, start, start))  # real == poison: the latents a run starts from
            for t in s.dd_dev + s.db_dev:
                self.gated.append(Gated(t, t.clone(), torch.zeros_like(t)))
        geo = self.syns[0].geo
        self.full = (1 << geo.n) - 1
        if kind == "follow":
            rng = np.random.default_rng(9)
            self.motion = _dev(rng.uniform(-3.0, 3.0, size=(2, geo.H, geo.W)).astype(np.float32))

    def open(self):
        from cool_chic_amd import RdoqStep

        step = RdoqStep(0)
        for s in self.syns:
            s.add_to(step)
        if self.kind == "follow":
            step.follow(0, 1, 0, self.motion.data_ptr(), target=1, global_flow=(1, -2, 0, 0), warp_filter_size=8, owner=self.motion)
        return step

    def call(self, h, stream):
        from cool_chic_amd._lib import check, lib

        n = len(self.syns)
        kD, kR = [s.kD for s in self.syns], [s.kR for s in self.syns]
        if self.kind == "rounds1":
            dbl = C.c_double * n
            check(lib().ccd_rdoq_step(h._h, dbl(*kD), dbl(*kR), dbl(*([0.0] * n)), (C.c_uint64 * n)(*([self.full] * n)),
                                      C.c_void_p(stream or None)), "ccd_rdoq_step")
        else:
            h.step(kD, kR, [0.0] * n, [self.full] * n, stream, rounds=self.rounds)

    def wait(self, h, stream):
        h.wait(stream)

    def read(self, h):
        import torch

        geo = self.syns[0].geo
        out = []
        for k, s in enumerate(self.syns):
            out.append((s.buf.clone(), tuple(h.result(k)), [torch.as_tensor(h.moves(k, g), device="cuda").clone() for g in range(geo.n)]))
        return out

    def early(self, h):
        return [s.buf for s in self.syns]

    def early_result(self, snaps, result):
        return canon(snaps)


class IScoreCase(Case):
    """InterScore.run over one handle with a P frame of 16 x 24, 4:2:0, 8 bits, 8 taps and a B frame of 37 x 53, RGB, 10 bits,
    4 taps (tests/test_inter_score.py's _Frame), each with a residue item, a motion item and a reference item.  `group`: which of
    the inputs - residue outputs, motion outputs, reference planes, source planes - are gated; the others hold the real input."""

    foreign_wait = True
    GROUPS = ("residue", "motion", "references", "sources")

    def __init__(self, group):
        from test_inter_score import _Frame

        self.name = f"iscore_{group}"

        def frames(seed):
            return [_Frame(1, 16, 24, 1, 8, 8, "subpixel", [1, -2, 0, 0], seed=[seed, 1]),
                    _Frame(2, 37, 53, 0, 10, 4, "subpixel", [-2, 1, 2, -1], seed=[seed, 2])]

        self.frames, spare = frames(31), frames(32)
        self.gated = []
        self.items = []  # per frame: (residue candidate, motion candidate, reference-0 candidate planes)
        for f, p in zip(self.frames, spare):
            cand = [f.outputs(0, 0), f.outputs(1, 0), f._planes([t.cpu().numpy() for t in p.refs[0]])]
            cand_p = [p.outputs(0, 1), p.outputs(1, 1), f._planes([t.cpu().numpy()[::-1, ::-1].copy() for t in p.refs[0]])]
            self.items.append(cand)
            pairs = {"residue": [(f.residue, p.residue), (cand[0], cand_p[0])], "motion": [(f.motion, p.motion), (cand[1], cand_p[1])],
                     "references": [(a, b) for ra, rb in zip(f.refs, p.refs) for a, b in zip(ra, rb)] + list(zip(cand[2], cand_p[2])),
                     "sources": list(zip(f.src, p.src))}[group]
            for live, poison in pairs:
                self.gated.append(Gated(live, live.clone(), poison))

    def open(self):
        from cool_chic_amd import InterScore

        s = InterScore(0)
        for f, (res, mot, ref0) in zip(self.frames, self.items):
            k = f.add_to(s)
            s.add(k, 0, res.data_ptr(), owner=res)
            s.add(k, 1, mot.data_ptr(), owner=mot)
            s.add_refs(k, [t.data_ptr() for t in ref0], None, owner=ref0)
        return s

    def call(self, h, stream):
        h.run(stream)

    def wait(self, h, stream):
        h.wait(stream)

    def read(self, h):
        return ([h.frame_sse(k) for k in range(2)], [h.sse(i) for i in range(6)])


class ReconstructCase(Case):
    """ccd_inter_reconstruct through tests/test_inter_reconstruct.py's launcher with a stream argument: a P or a B frame of
    37 x 53 (RGB, 10 bits, sinc-8).  Residue, motion and references are gated.  The header does not say that the call only
    enqueues, so a call that synchronised would be conclusive as it is."""

    has_handle = False
    enqueues = False

    def __init__(self, frame_type):
        import test_inter_reconstruct as T

        self.name = f"reconstruct_{'pb'[frame_type - 1]}"
        self.T = T
        self.c = dict(id=self.name, n_taps=8, frame_type=frame_type, bitdepth=10, fdt=0, h=37, w=53, flow="subpixel",
                      gflow=[1, -2, -3, 1], seed=4000 + frame_type)
        real = T._device_inputs(self.c, T.case_data(self.c))
        poison = T._device_inputs(self.c, T.case_data(dict(self.c, seed=5000 + frame_type)))
        self.out = real.out
        flat = lambda d: [d.residue, d.motion] + [p for r in d.refs for p in r]  # noqa: E731
        self.gated = _gate_all(flat(real), flat(poison))
        live = [g.live for g in self.gated]
        self.inputs = T._Inputs(live[0], live[1], [live[2:5]] + ([live[5:8]] if frame_type == 2 else []), self.out)

    def call(self, h, stream):
        self.T._launch(self.c, self.inputs, stream)

    def wait(self, h, stream):
        stream_sync(stream)

    def read(self, h):
        return [p.clone() for p in self.out]

    def early(self, h):
        return self.out


_CASES = {}


def case(name, oracle=None):
    """The case of that name, built once (GPU)."""
    if name not in _CASES:
        if name.startswith(("enc_", "decode_")):
            if "rgb192" not in _CASES:
                _CASES["rgb192"] = _Rgb192(oracle)
            rgb = _CASES["rgb192"]
            _CASES[name] = DecodeCase(rgb) if name == "decode_given" else EncCase(rgb, name[len("enc_"):])
        elif name.startswith("rate"):
            _CASES[name] = RateCase(name == "rate_total")
        elif name.startswith("quality_"):
            _CASES[name] = QualityCase(name[len("quality_"):])
        elif name.startswith("png_"):
            _CASES[name] = PngCase(int(name[-1]), "batch" in name)
        elif name.startswith("dsens_"):
            _CASES[name] = DsensCase(name[len("dsens_"):])
        elif name.startswith("rdoq_"):
            _CASES[name] = RdoqCase(name[len("rdoq_"):])
        elif name.startswith("iscore_"):
            _CASES[name] = IScoreCase(name[len("iscore_"):])
        elif name.startswith("reconstruct_"):
            _CASES[name] = ReconstructCase(1 + "pb".index(name[-1]))
        else:
            raise KeyError(name)
        assert _CASES[name].name == name
    return _CASES[name]


CASE_NAMES = sorted({n for names in COVERAGE.values() for n in names})
# what the header promises of each case (the classes say the same; this table needs no device)
NO_HANDLE = ("rate", "rate_total", "reconstruct_p", "reconstruct_b")
MAY_SYNCHRONISE = ("reconstruct_p", "reconstruct_b")
EARLY = ("rate", "rate_total", "png_level0", "png_level1", "png_batch_level0", "png_batch_level1", "decode_given", "rdoq_rounds1",
         "rdoq_rounds8", "rdoq_follow", "reconstruct_p", "reconstruct_b")
# one case per handle whose wait takes a stream: the wait on a stream other than the run's
FOREIGN_WAIT = ("quality_decoded", "png_level0", "png_batch_level1", "enc_measure", "decode_given", "dsens_inter_p_residue", "rdoq_rounds8",
                "iscore_motion")
