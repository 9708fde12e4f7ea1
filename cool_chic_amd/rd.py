"""RdEvaluator: rate, distortion and D + lambda R of candidate (latents, networks) on one MI355X, without a serial chain.

The three device meters behind one call: the candidates' planes come from the float path over GIVEN
latents (DecodeBatch.add_latents*, ccd_batch_add_latents), their rate from the rate meter (EncodeBatch.measure) and their
distortion from the quality meter (QualityMeter.score_planes).  Neither the range encoder's nor the range decoder's chain runs.

The cost has the shape of the reference's loss (training/loss.py:158 loss_function: distortion + lmbda * rate in bits per
pixel, the frame's MSE weighted by plane size for 4:2:0, loss.py:88-118):

    mse      = sum of squared errors over all planes / (n_samples * (2^bitdepth - 1)^2)
    bits     = total_bits + 8 * (n_bytes_nn + n_bytes_header)
    cost     = mse + lmbda * bits / n_pixels            (n_pixels: the luma size)

It differs from the reference's in two stated ways.  The distortion is that of the INTEGER planes a decoder writes (the
reference trains on the float synthesis output and only its final test pass quantises to the bit depth), and the rate of the
latents is the decoder's exact integer ARM priced as model bits, 24 - log2(interval width) per symbol, not the float rate
estimate of training and not the coded bytes (the payload is 0 to 3 words above ceil(total_bits / 32)).  The
cost is computed on the host in float64 from the device's exact integer squared error and its total_bits.

A candidate of a frame that P / B frames predict from is also priced through them (cost_with_dependents):

    cost_with_dependents = cost + sum over the dependents d of  sse_d / (n_samples_d * (2^bitdepth_d - 1)^2)

the GOP's summed per-frame cost with the dependents' own bits left out - the candidate does not change them - where sse_d is the
squared error of dependent d reconstructed against the candidate's planes (InterScore.add_refs).  float64, in list order.

Intra frames only: one cool-chic per frame.  P / B frames (two cool-chics and a reconstruction) are not evaluated here;
ccd_batch_add_latents itself takes any cool-chic."""
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from ._handle import dev_ptr
from ._lib import CCHeader
from .batch import FRAME_DATA_TYPES, DecodeBatch
from .dsens import SENTINEL, DistortionDeltas
from .encoder import EncodeBatch, SlotRate
from .io import FrameData
from .quality import FrameQuality, QualityMeter, _frame_planes, scored_frame_type
from .rdoq import RdoqStep, SlotMaps, StepResult, check_lambda, grid_mask, run_step


class Candidate(NamedTuple):
    rate: SlotRate
    quality: FrameQuality
    mse: float
    bits: float
    cost: float


class StepReport(NamedTuple):
    """One candidate in one step of RdEvaluator.descend: what it was before the step, and what the step did to it."""
    before: Candidate
    step: StepResult


def rd_cost(sse: Sequence[int], n: Sequence[int], bitdepth: int, total_bits: float, n_bytes_nn: int, n_bytes_header: int,
            n_pixels: int, lmbda: float):
    """(mse, bits, cost) in float64 from the device's integers: the definition in this module's docstring."""
    maxv = float(2 ** bitdepth - 1)
    mse = float(sum(int(v) for v in sse)) / (float(sum(int(v) for v in n)) * maxv * maxv)
    bits = float(total_bits) + 8.0 * float(int(n_bytes_nn) + int(n_bytes_header))
    return mse, bits, mse + float(lmbda) * bits / float(n_pixels)


def cost_with_dependents(own, dependents) -> float:
    """own: rd_cost's (mse, bits, cost) of the frame; dependents: [(sse[3], n[3], bitdepth)] of the frames that predict from it,
    each reconstructed against the frame's planes, in registration order.  own.cost plus every dependent's mse (rd_cost's
    definition), summed in float64 in list order: the definition in this module's docstring."""
    cost = float(own[2])
    for sse, n, bitdepth in dependents:
        maxv = float(2 ** int(bitdepth) - 1)
        cost += float(sum(int(v) for v in sse)) / (float(sum(int(v) for v in n)) * maxv * maxv)
    return cost


def move_scales(n_samples: int, bitdepth: int, n_pixels: int, lmbda: float):
    """(kD, kR): what one unit of squared error and one bit add to rd_cost's cost."""
    maxv = float(2 ** bitdepth - 1)
    return 1.0 / (float(n_samples) * maxv * maxv), float(lmbda) / float(n_pixels)


def move_cost_map(dd: torch.Tensor, db: torch.Tensor, n_samples: int, bitdepth: int, n_pixels: int, lmbda: float) -> torch.Tensor:
    """rd_cost's definition applied to the +-1 moves of a grid (dd: int64 distortion deltas, db: float64 rate deltas), in float64;
    +inf where the move leaves [-64, 63]."""
    maxv = float(2 ** bitdepth - 1)
    cost = dd.to(torch.float64) / (float(n_samples) * maxv * maxv) + float(lmbda) * db / float(n_pixels)
    return torch.where((dd == SENTINEL) | torch.isinf(db), torch.full_like(cost, float("inf")), cost)


class RdEvaluator:
    """add() candidates, then evaluate(lmbda): one DecodeBatch of given latents, one EncodeBatch over the same device grids,
    one scoring.  evaluate() may be called again (another lambda, or after device latents were changed in place)."""

    def __init__(self, device: int = 0, n_probe_slots: int = 16):
        """n_probe_slots: float-path passes in flight per candidate when distortion deltas are asked for (DistortionDeltas)."""
        self.device = int(device)
        self._n_probe_slots = int(n_probe_slots)
        self._dd = None             # DistortionDeltas over the candidates, made when first asked for
        self._jobs: List[tuple] = []  # (arch, bytes_nn) per candidate, for it
        self._dependents: List[List[dict]] = []  # per candidate: the add_dependent() calls, for it
        self._rdoq = None           # RdoqStep over the candidates, made by the first descend()
        self._caller_ptrs: List[Optional[List[int]]] = []  # the caller's device latents per candidate; None: host arrays
        self._dec = DecodeBatch(self.device)
        self._enc = EncodeBatch(self.device)
        self._meter = QualityMeter(self.device)
        self._sources: List[List[torch.Tensor]] = []
        self._frames: List[FrameData] = []

    def close(self):
        if self._rdoq is not None:
            self._rdoq.close()
            self._rdoq = None
        if self._dd is not None:
            self._dd.close()
            self._dd = None
        self._enc.close()
        self._dec.close()
        self._meter.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return len(self._frames)

    def add(self, arch: CCHeader, bytes_nn: bytes, latents_or_ptrs: Sequence[Union[np.ndarray, int]], source: FrameData, owner=None) -> int:
        """A candidate: host latent arrays (uploaded once, here) or device addresses (int8 [h][w] per grid, read at every
        evaluate(); `owner` keeps them alive), and the frame it is scored against."""
        fdt = scored_frame_type(source)
        on_device = all(isinstance(x, (int, np.integer)) for x in latents_or_ptrs)
        if on_device:
            slot = self._dec.add_latents_device(arch, bytes_nn, latents_or_ptrs, source.bitdepth, fdt, owner=owner)
        else:
            slot = self._dec.add_latents(arch, bytes_nn, latents_or_ptrs, source.bitdepth, fdt)
        h = self._dec.header(slot)
        if tuple(h.img_size) != tuple(source.img_size):
            raise ValueError(f"the candidate decodes to {h.img_size[0]}x{h.img_size[1]}, its source is {source.img_size[0]}x{source.img_size[1]}")
        # the rate meter reads the grids where the decode batch keeps them: host latents crossed PCIe once
        self._enc.add_device(arch, bytes_nn, self._dec.latent_ptrs(slot), owner=self._dec)
        self._sources.append(_frame_planes(source, torch.device(f"cuda:{self.device}")))
        self._frames.append(source)
        self._jobs.append((arch, bytes_nn))
        self._dependents.append([])
        self._caller_ptrs.append([int(p) for p in latents_or_ptrs] if on_device else None)
        return slot

    # -- what a caller that steps the candidates itself needs of one (rd_gop.GopDescent)
    def planes(self, slot: int) -> List[torch.Tensor]:
        """The integer device planes the candidate decodes to: library memory at a fixed address, rewritten by every evaluate()."""
        return [torch.as_tensor(self._dec.plane_device(int(slot), p), device=f"cuda:{self.device}") for p in range(3)]

    def architecture(self, slot: int) -> CCHeader:
        return self._jobs[int(slot)][0]

    def source(self, slot: int) -> FrameData:
        return self._frames[int(slot)]

    def caller_latent_ptrs(self, slot: int) -> Optional[List[int]]:
        """The caller's device latents the candidate was added with; None: it was added from host arrays."""
        return self._caller_ptrs[int(slot)]

    def move_scales(self, slot: int, lmbda: float):
        """move_scales() of the candidate's frame: (kD, kR) of an RdoqStep over its maps."""
        f = self._frames[int(slot)]
        return move_scales(sum(int(t.numel()) for t in self._sources[int(slot)]), f.bitdepth, f.n_pixels, lmbda)

    def add_dependent(self, slot: int, frame_type: int, which: int, residue_ptr: int, motion_ptr: int, source_ptrs: Sequence[int],
                      other_ref_ptrs: Optional[Sequence[int]] = None, global_flow: Sequence[int] = (0, 0, 0, 0),
                      warp_filter_size: int = 8, owner=None) -> None:
        """A P / B frame that predicts from candidate `slot` as its reference `which` (DistortionDeltas.add_dependent, DESIGN.md
        4.16): recorded, and handed to the DistortionDeltas handle when evaluate(distortion_deltas=True) makes or extends it.
        Changes nothing that evaluate() returns; dependent_delta_map() and cost_delta_map(dependents=True) read what it adds."""
        if not 0 <= int(slot) < len(self._frames):
            raise IndexError(f"no candidate {slot}")
        dep = dict(frame_type=frame_type, which=which, residue_ptr=residue_ptr, motion_ptr=motion_ptr, source_ptrs=list(source_ptrs),
                   other_ref_ptrs=None if other_ref_ptrs is None else list(other_ref_ptrs), global_flow=list(global_flow),
                   warp_filter_size=warp_filter_size, owner=owner)
        self._dependents[int(slot)].append(dep)
        if self._dd is not None and int(slot) < len(self._dd):
            self._dd.add_dependent(int(slot), **dep)

    def evaluate(self, lmbda: float, ms_ssim: bool = False, rate_deltas: bool = False, distortion_deltas: bool = False) -> List[Candidate]:
        """rate_deltas: the rate comes from EncodeBatch.measure_deltas, which leaves the same numbers and, for
        rate_delta_map(), what every latent's +-1 would do to them.  distortion_deltas: a DistortionDeltas run over the same
        device grids follows, for distortion_delta_map() and cost_delta_map(); the candidates returned are the same."""
        n = len(self._frames)
        if n == 0:
            return []
        st = torch.cuda.current_stream(self.device).cuda_stream
        self._dec.run(st)           # ingest of device latents, then the float path: the grids are in the arenas behind this
        if rate_deltas:             # same stream: reads the arenas' grids
            self._enc.measure_deltas(st)
        else:
            self._enc.measure(st)
        decoded = [[torch.as_tensor(self._dec.plane_device(s, p), device=f"cuda:{self.device}") for p in range(3)] for s in range(n)]
        self._meter.score_planes_async(decoded, self._sources, [f.bitdepth for f in self._frames], ms_ssim, stream=st)
        results = self._meter.finish()
        self._dec.wait(st)          # a refused device latent raises here (CCD_ERR_VALUE)
        self._enc.wait(st)
        if distortion_deltas:
            self.run_distortion_deltas()
        out = []
        for s, (r, f) in enumerate(zip(results, self._frames)):
            rate = self._enc.rate(s)
            q = FrameQuality.from_result(r, f.bitdepth, f.frame_data_type)
            mse, bits, cost = rd_cost(q.sse, q.n, f.bitdepth, rate.total_bits, rate.n_bytes_nn, rate.n_bytes_header, f.n_pixels, lmbda)
            out.append(Candidate(rate, q, mse, bits, cost))
        return out

    def run_distortion_deltas(self) -> None:
        """The DistortionDeltas run of evaluate(distortion_deltas=True) on its own, over the grids as the last evaluate() ingested
        them: own maps and, for candidates with add_dependent() frames, dependent maps - which read the dependents' float outputs
        as they are NOW, so a caller that evaluates the dependents between the two (rd_gop.GopDescent) gets maps of the current
        state of both."""
        n = len(self._frames)
        st = torch.cuda.current_stream(self.device).cuda_stream
        # reads the grids in the decode batch's arenas and the sources the meter read
        if self._dd is None:
            self._dd = DistortionDeltas(self.device, self._n_probe_slots)
        for s in range(len(self._dd), n):
            arch, bytes_nn = self._jobs[s]
            f = self._frames[s]
            self._dd.add(arch, bytes_nn, self._dec.latent_ptrs(s), [t.data_ptr() for t in self._sources[s]], f.bitdepth,
                         FRAME_DATA_TYPES.index(f.frame_data_type), owner=self._dec)
            for dep in self._dependents[s]:
                self._dd.add_dependent(s, **dep)
        self._dd.run(st)
        self._dd.wait(st)

    def rate_delta_map(self, slot: int, grid: int):
        """After evaluate(rate_deltas=True): EncodeBatch.delta_map of the candidate (device, float32 [2][h][w])."""
        return self._enc.delta_map(slot, grid)

    def distortion_delta_map(self, slot: int, grid: int):
        """After evaluate(distortion_deltas=True): DistortionDeltas.delta_map of the candidate (device, int64 [2][h][w])."""
        if self._dd is None:
            raise RuntimeError("no evaluate(distortion_deltas=True) has run")
        return self._dd.delta_map(slot, grid)

    def dependent_delta_map(self, slot: int, grid: int):
        """After evaluate(distortion_deltas=True) of a candidate with add_dependent() frames: DistortionDeltas.dep_delta_map
        (device, int64 [2][h][w]): what the move does to the squared error of the frames that predict from the candidate."""
        if self._dd is None:
            raise RuntimeError("no evaluate(distortion_deltas=True) has run")
        return self._dd.dep_delta_map(slot, grid)

    def cost_delta_map(self, slot: int, grid: int, lmbda: float, dependents: bool = False) -> torch.Tensor:
        """After evaluate(rate_deltas=True, distortion_deltas=True): what moving the latent (y, x) of `grid` by -1 (plane 0) or
        +1 (plane 1) does to the candidate's cost, the module's definition applied to the move - float64 [2][h][w] on the device,

            dD / (n_samples * (2^bitdepth - 1)^2) + lmbda * dBits / n_pixels

        and +inf where the move leaves [-64, 63].  dependents=True: dD is the own delta plus dependent_delta_map's - the frames
        of one video have one size, so one unit of squared error weighs the same in each - and +inf also at its conflicts."""
        dev = f"cuda:{self.device}"
        f = self._frames[slot]
        n_samples = sum(int(t.numel()) for t in self._sources[slot])
        dd = torch.as_tensor(self.distortion_delta_map(slot, grid), device=dev)
        if dependents:
            dep = torch.as_tensor(self.dependent_delta_map(slot, grid), device=dev)
            dd = torch.where((dd == SENTINEL) | (dep == SENTINEL), torch.full_like(dd, SENTINEL), dd + dep)
        db = torch.as_tensor(self.rate_delta_map(slot, grid), device=dev).to(torch.float64)
        return move_cost_map(dd, db, n_samples, f.bitdepth, f.n_pixels, lmbda)

    def descend(self, lmbda: float, max_steps: int, min_gain: float = 0.0, grids: Optional[Sequence[int]] = None,
                rounds: int = 1) -> List[List[StepReport]]:
        """Requantisation by descent.  Per step: evaluate(lmbda, rate_deltas=True, distortion_deltas=True), then
        one RdoqStep over the evaluator's own device maps that moves latents of the candidates IN PLACE by +-1 where that lowers
        the cost by more than `min_gain` and the moves do not interact.  `grids`: the grids that may move (all by default).
        With every grid admitted a step of a real picture is usually ONE move: a candidate of the coarsest grids reaches the
        whole picture, is worth thousands of squared-error units and so beats and blocks everything else.  Pass the fine grids
        (for instance grids=(0, 1, 2)) for steps of hundreds of moves, and admit the coarse ones in a later call.
        `rounds`: rounds of selection per step (RdoqStep.step; 1 .. 64, 8 is a sensible value): the maps of one evaluate() then
        yield every move that a walk over the candidates in key order would take, not only the winners of the first contest,
        a few times as many.  The advice about the coarse grids still holds: a coarse candidate with the BEST key still owns the
        whole raster.  What changes is that a coarse candidate that LOSES no longer blocks the rest.
        Stops when no candidate moved or after `max_steps` steps; returns one list of StepReport per step (one per candidate:
        the candidate before the step, and what the step did).  After a step the cost of candidate s is before.cost + step.d_cost
        (its distortion part exactly, its rate part within the rate deltas' bound).

        Every candidate must have been added with DEVICE latents: they are the caller's memory, changed in place and seen by the
        next evaluate().  A candidate added from host arrays raises ValueError before anything runs."""
        n = len(self._frames)
        for s, ptrs in enumerate(self._caller_ptrs):
            if ptrs is None:
                raise ValueError(f"candidate {s} was added from host arrays: descend() moves device latents the caller owns")
        check_lambda(lmbda, min_gain)
        if n == 0:
            return []
        st = torch.cuda.current_stream(self.device).cuda_stream
        if self._rdoq is None:
            self._rdoq = RdoqStep(self.device)
        for s in range(len(self._rdoq), n):
            f = self._frames[s]
            self._rdoq.add(self._jobs[s][0], FRAME_DATA_TYPES.index(f.frame_data_type), self._caller_ptrs[s])
        fixed = [(*self.move_scales(s, lmbda), grid_mask(int(arch.n_grids), grids), range(int(arch.n_grids)))
                 for s, (arch, _) in enumerate(self._jobs)]
        reports: List[List[StepReport]] = []
        for _ in range(int(max_steps)):
            before = self.evaluate(lmbda, rate_deltas=True, distortion_deltas=True)  # (the maps' addresses are those of this run)
            slots = [SlotMaps(kD, kR, mask, [dev_ptr(self._dd.delta_map(s, g)) for g in gs], [dev_ptr(self._enc.delta_map(s, g)) for g in gs])
                     for s, (kD, kR, mask, gs) in enumerate(fixed)]
            results = run_step(self._rdoq, st, slots, min_gain, rounds)
            reports.append([StepReport(b, r) for b, r in zip(before, results)])
            if not any(r.n_moves for r in results):
                break
        return reports

    def step_moves(self, slot: int, grid: int):
        """After descend(): the last step's move (-1, 0, +1) at every latent of the grid (device, int8 [h][w])."""
        if self._rdoq is None:
            raise RuntimeError("no descend() has run")
        return self._rdoq.moves(slot, grid)
