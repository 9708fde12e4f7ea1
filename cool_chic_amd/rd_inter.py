"""InterRdEvaluator: rate, distortion and D + lambda R of P / B frames on one MI355X, and their requantisation by descent
(DESIGN.md section 4.15).  The counterpart of rd.RdEvaluator for frames that are decoded from TWO cool-chics, residue and motion,
and a reconstruction against reference frames (ccd_inter_reconstruct).

Per frame one evaluation is: the float outputs of both cool-chics from given latents (one DecodeBatch, no integer planes of their
own, as the decoder adds them), ccd_inter_reconstruct for the frame's planes, QualityMeter for their squared error,
EncodeBatch.measure[_deltas] over both cool-chics.  The cost is rd.rd_cost with the model bits, network bytes and cool-chic
header bytes of BOTH cool-chics summed.

The distortion deltas of a cool-chic are taken with the other one's output held fixed (DistortionDeltas.add_inter): the
reconstruction is pointwise, so the footprints, lattice passes and influence boxes of an intra cool-chic hold for either.  A
descent step of one role moves that cool-chic alone; inside one cool-chic the influence boxes make the chosen moves independent,
and after the step the frame's squared error has changed by exactly the sum of the chosen entries.

A JOINT step (descend(joint=True)) moves both.  A sample of the frame reads both cool-chics' outputs at its own position only, and
both have the frame's size and format, so their influence boxes lie in one raster of cells: a residue latent and a motion latent
whose boxes share no cell change disjoint sets of samples, each map was taken with the partner as it is outside its own box, and
the frame's squared error changes by the sum of the two entries.  The two rate models read nothing of each other, so the bits add.
RdoqStep.link lets the two slots of a frame compete for the cells of one raster."""
import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._handle import dev_ptr
from ._lib import CCHeader, check, lib
from .batch import FRAME_DATA_TYPES, DecodeBatch
from .dsens import DistortionDeltas
from .encoder import EncodeBatch, SlotRate
from .io import FrameData
from .quality import FrameQuality, QualityMeter, _frame_planes, scored_frame_type
from .rd import move_cost_map, move_scales, rd_cost
from .rdoq import RdoqStep, SlotMaps, StepResult, check_lambda, grid_mask, run_step

ROLES = ("residue", "motion")


def _role(role: Union[str, int]) -> int:
    if role in ROLES:
        return ROLES.index(role)
    if role in (0, 1):
        return int(role)
    raise ValueError(f"role must be 'residue' / 'motion' (0 / 1), not {role!r}")


def inter_frame_type(frame_type: Union[str, int]) -> int:
    """1 for 'P' / 1, 2 for 'B' / 2: the number of reference frames."""
    ft = {"P": 1, "B": 2}.get(frame_type, frame_type)
    if ft not in (1, 2):
        raise ValueError(f"frame_type must be 'P' / 'B' (1 / 2), not {frame_type!r}")
    return ft


def reference_planes(ft: int, references: Sequence, device: torch.device) -> List[List[torch.Tensor]]:
    """The frame's `ft` references as device planes: a FrameData is uploaded, three planes are taken as they are."""
    if len(references) < ft:
        raise ValueError(f"a {'PB'[ft - 1]} frame needs {ft} reference frame(s)")
    return [_frame_planes(r, device) if isinstance(r, FrameData) else [p for p in r] for r in list(references)[:ft]]


def padded_global_flow(global_flow: Sequence[int]) -> List[int]:
    return ([int(v) for v in global_flow] + [0, 0, 0, 0])[:4]


class InterCandidate(NamedTuple):
    rates: Tuple[SlotRate, SlotRate]   # residue, motion
    quality: FrameQuality
    mse: float
    bits: float                        # of both cool-chics: model bits + 8 * (network and cool-chic header bytes)
    cost: float


class InterStepReport(NamedTuple):
    """One frame in one step of InterRdEvaluator.descend: the frame before the step, the role that could move, what the step did."""
    before: InterCandidate
    role: str
    step: StepResult


class InterJointStepReport(NamedTuple):
    """One frame in one JOINT step of InterRdEvaluator.descend(joint=True): the frame before the step and what the step did in
    each cool-chic, (residue, motion)."""
    before: InterCandidate
    steps: Tuple[StepResult, StepResult]


class _Frame(NamedTuple):
    frame_type: int                    # 1 P, 2 B
    archs: Tuple[CCHeader, CCHeader]
    nns: Tuple[bytes, bytes]
    caller_ptrs: Tuple[List[int], List[int]]
    refs: List[List[torch.Tensor]]
    global_flow: List[int]
    warp_filter_size: int
    source: FrameData
    src: List[torch.Tensor]
    planes: List[torch.Tensor]         # what the last evaluate() reconstructed


class InterRdEvaluator:
    """add() frames, then evaluate(lmbda) or descend(...).  Frame f owns the slots 2 f (residue) and 2 f + 1 (motion) of every
    handle inside."""

    def __init__(self, device: int = 0, n_probe_slots: int = 16):
        self.device = int(device)
        self._n_probe_slots = int(n_probe_slots)
        self._dec = DecodeBatch(self.device)
        self._enc = EncodeBatch(self.device)
        self._meter = QualityMeter(self.device)
        self._dd: Dict[int, DistortionDeltas] = {}   # per role: a step reads the moving role's maps only
        self._dd_frames: Dict[int, int] = {0: 0, 1: 0}
        self._rdoq: Optional[RdoqStep] = None
        self._n_linked = 0                           # frames whose motion slot is linked to the residue slot (descend(joint=True))
        self._frames: List[_Frame] = []
        self._owners = []

    def close(self):
        if self._rdoq is not None:
            self._rdoq.close()
            self._rdoq = None
            self._n_linked = 0
        for d in self._dd.values():
            d.close()
        self._dd = {}
        self._enc.close()
        self._dec.close()
        self._meter.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return len(self._frames)

    def add(self, frame_type: Union[str, int], residue, motion, references: Sequence, global_flow: Sequence[int], warp_filter_size: int,
            source: FrameData, owner=None) -> int:
        """A P / B frame.  residue, motion: (arch, bytes_nn, device addresses of the int8 latent grids) - the caller's memory, read
        at every evaluate() and moved in place by descend(); `owner` keeps it alive.  references: one (P) or two (B) reference
        frames, each a FrameData or three integer device planes (torch tensors, kept and read at every evaluate()); source: the
        frame it is scored against, which also gives the bit depth and the sample format.  Returns the frame index."""
        ft = inter_frame_type(frame_type)
        scored_frame_type(source)
        dev = torch.device(f"cuda:{self.device}")
        refs = reference_planes(ft, references, dev)
        src = _frame_planes(source, dev)
        for planes in refs:
            if [tuple(p.shape) for p in planes] != [tuple(p.shape) for p in src] or any(p.dtype != s.dtype or not p.is_cuda or
                                                                                       not p.is_contiguous() for p, s in zip(planes, src)):
                raise ValueError("a reference must have the frame's plane sizes and sample type, on the device")
        archs, nns, ptrs = [], [], []
        for role, (arch, nn, latent_ptrs) in enumerate((residue, motion)):
            if not all(isinstance(x, (int, np.integer)) for x in latent_ptrs):
                raise ValueError("only device latents are accepted: descend() moves them in place")
            if tuple(arch.img_size) != tuple(source.img_size):
                raise ValueError(f"the {ROLES[role]} cool-chic decodes to {arch.img_size[0]}x{arch.img_size[1]}, the frame is "
                                 f"{source.img_size[0]}x{source.img_size[1]}")
            want = (5 if ft == 2 else 4) if role == 0 else (4 if ft == 2 else 2)
            if arch.out_channels not in (0, want):  # (0: an arch without derived geometry; ccd_dsens_add_inter checks it then)
                raise ValueError(f"the {ROLES[role]} cool-chic of a {'PB'[ft - 1]} frame has {want} output channels, not {arch.out_channels}")
            archs.append(arch); nns.append(bytes(nn)); ptrs.append([int(p) for p in latent_ptrs])
        for role in range(2):
            slot = self._dec.add_latents_device(archs[role], nns[role], ptrs[role], 0, 0)
            # the rate meter reads the grids where the decode batch keeps them
            self._enc.add_device(archs[role], nns[role], self._dec.latent_ptrs(slot), owner=self._dec)
        planes = [torch.empty_like(p) for p in src]
        self._frames.append(_Frame(ft, tuple(archs), tuple(nns), tuple(ptrs), refs, padded_global_flow(global_flow), int(warp_filter_size),
                                   source, src, planes))
        self._owners.append(owner)
        return len(self._frames) - 1

    def planes(self, frame: int) -> List[torch.Tensor]:
        """The integer device planes of the frame as the last evaluate() reconstructed them."""
        return self._frames[frame].planes

    # -- what a caller that steps the frames itself needs of one (rd_gop.GopDescent)
    def frame(self, frame: int) -> _Frame:
        """What add() recorded of the frame: type, architectures, the caller's latents, references, global flow, filter size,
        source planes."""
        return self._frames[int(frame)]

    def output_ptr(self, frame: int, role) -> int:
        """The device address of the float output of the role's cool-chic: library memory at a fixed address, rewritten by every
        evaluate()."""
        return dev_ptr(self._dec.output_device(2 * int(frame) + _role(role)))

    def frame_data_type_index(self, frame: int) -> int:
        return self._fdt(self._frames[int(frame)])

    def move_scales(self, frame: int, lmbda: float):
        """rd.move_scales of the frame: (kD, kR) of an RdoqStep over the maps of either cool-chic."""
        f = self._frames[int(frame)]
        return move_scales(sum(int(t.numel()) for t in f.src), f.source.bitdepth, f.source.n_pixels, lmbda)

    def _fdt(self, f: _Frame) -> int:
        return FRAME_DATA_TYPES.index(f.source.frame_data_type)

    def _reconstruct(self, k: int, st: int):
        f = self._frames[k]
        h, w = f.source.img_size

        def ptrs(planes):
            return (C.c_void_p * 3)(*[p.data_ptr() for p in planes])

        out = [dev_ptr(self._dec.output_device(2 * k + r)) for r in range(2)]
        check(lib().ccd_inter_reconstruct(self.device, C.c_void_p(st or None), f.frame_type, h, w, f.source.bitdepth, self._fdt(f),
                                          C.c_void_p(out[0]), C.c_void_p(out[1]), ptrs(f.refs[0]), ptrs(f.refs[1]) if f.frame_type == 2 else None,
                                          (C.c_int32 * 4)(*f.global_flow), f.warp_filter_size, ptrs(f.planes)), "ccd_inter_reconstruct")

    def _deltas(self, role: int) -> DistortionDeltas:
        if role not in self._dd:
            self._dd[role] = DistortionDeltas(self.device, self._n_probe_slots)
        d = self._dd[role]
        for k in range(self._dd_frames[role], len(self._frames)):
            f = self._frames[k]
            partner = dev_ptr(self._dec.output_device(2 * k + 1 - role))
            d.add_inter(f.archs[role], f.nns[role], self._dec.latent_ptrs(2 * k + role), [t.data_ptr() for t in f.src], f.source.bitdepth,
                        self._fdt(f), f.frame_type, role, partner, [t.data_ptr() for t in f.refs[0]],
                        [t.data_ptr() for t in f.refs[1]] if f.frame_type == 2 else None, f.global_flow, f.warp_filter_size, owner=self._dec)
        self._dd_frames[role] = len(self._frames)
        return d

    def evaluate(self, lmbda: float, rate_deltas: bool = False, distortion_deltas: bool = False,
                 roles: Sequence[Union[str, int]] = ROLES) -> List[InterCandidate]:
        """One InterCandidate per frame.  rate_deltas: EncodeBatch.measure_deltas in place of measure (same numbers, and the maps
        of rate_delta_map()).  distortion_deltas: a DistortionDeltas run per role of `roles` follows - two slots per frame, each
        with the other cool-chic's device output as its partner - for distortion_delta_map() and cost_delta_map()."""
        n = len(self._frames)
        if n == 0:
            return []
        st = torch.cuda.current_stream(self.device).cuda_stream
        self._dec.run(st)
        if rate_deltas:
            self._enc.measure_deltas(st)
        else:
            self._enc.measure(st)
        for k in range(n):
            self._reconstruct(k, st)
        self._meter.score_planes_async([f.planes for f in self._frames], [f.src for f in self._frames],
                                       [f.source.bitdepth for f in self._frames], False, stream=st)
        results = self._meter.finish()
        self._dec.wait(st)          # a refused device latent raises here (CCD_ERR_VALUE)
        self._enc.wait(st)
        if distortion_deltas:       # read the grids in the decode batch's arenas and its float outputs, as they are now
            for role in sorted({_role(r) for r in roles}):
                d = self._deltas(role)
                d.run(st)
                d.wait(st)
        out = []
        for k, (r, f) in enumerate(zip(results, self._frames)):
            rates = (self._enc.rate(2 * k), self._enc.rate(2 * k + 1))
            q = FrameQuality.from_result(r, f.source.bitdepth, f.source.frame_data_type)
            mse, bits, cost = rd_cost(q.sse, q.n, f.source.bitdepth, rates[0].total_bits + rates[1].total_bits,
                                      rates[0].n_bytes_nn + rates[1].n_bytes_nn, rates[0].n_bytes_header + rates[1].n_bytes_header,
                                      f.source.n_pixels, lmbda)
            out.append(InterCandidate(rates, q, mse, bits, cost))
        return out

    def rate_delta_map(self, frame: int, role, grid: int):
        """After evaluate(rate_deltas=True): device float32 [2][h][w] of the role's cool-chic."""
        return self._enc.delta_map(2 * int(frame) + _role(role), grid)

    def distortion_delta_map(self, frame: int, role, grid: int):
        """After evaluate(distortion_deltas=True): device int64 [2][h][w], the change of the FRAME's squared error."""
        r = _role(role)
        if r not in self._dd or int(frame) >= self._dd_frames[r]:
            raise RuntimeError("no evaluate(distortion_deltas=True) has covered this frame and role")
        return self._dd[r].delta_map(int(frame), grid)

    def cost_delta_map(self, frame: int, role, grid: int, lmbda: float) -> torch.Tensor:
        """RdEvaluator.cost_delta_map for one cool-chic of the frame: float64 [2][h][w] on the device,

            dD / (n_samples * (2^bitdepth - 1)^2) + lmbda * dBits / n_pixels

        and +inf where the move leaves [-64, 63]."""
        dev = f"cuda:{self.device}"
        f = self._frames[frame]
        n_samples = sum(int(t.numel()) for t in f.src)
        dd = torch.as_tensor(self.distortion_delta_map(frame, role, grid), device=dev)
        db = torch.as_tensor(self.rate_delta_map(frame, role, grid), device=dev).to(torch.float64)
        return move_cost_map(dd, db, n_samples, f.source.bitdepth, f.source.n_pixels, lmbda)

    def descend(self, lmbda: float, max_steps: int, min_gain: float = 0.0, grids=None,
                roles: Sequence[Union[str, int]] = ROLES, rounds: int = 1,
                joint: bool = False) -> List[List[Union[InterStepReport, InterJointStepReport]]]:
        """Requantisation by descent.  Per step: evaluate(lmbda, rate_deltas=True, distortion_deltas=True) for the moving role, then
        one RdoqStep that moves latents of THAT role's cool-chic of every frame in place by +-1 where the cost falls by more than
        `min_gain` and the moves do not interact; the other role's grid mask is 0.  The moving role alternates over `roles`; the
        descent stops after `max_steps` steps or when a full cycle over `roles` moved nothing.  `grids`: the grids that may move
        (all by default), or a dict of them per role.  Returns one list of InterStepReport (one per frame) per step.  After a step
        the frame's squared error is before + step.d_sse exactly; its bits within the rate deltas' bound of step.d_bits.
        `rounds`: rounds of selection per step (RdoqStep.step; 1 .. 64, 8 is a sensible value), as in RdEvaluator.descend: more
        moves from the maps of one evaluate().  A coarse candidate with the best key still owns the whole raster, so the advice
        to start with the fine grids holds; a coarse candidate that loses no longer blocks the rest.
        `joint`: every step moves BOTH roles.  The motion slot of every frame is linked to its residue slot (RdoqStep.link, once),
        a step is evaluate(lmbda, rate_deltas=True, distortion_deltas=True) for both roles and one RdoqStep whose selection is
        pairwise independent across the two cool-chics of a frame, and the descent stops after `max_steps` steps or after a step
        that moved nothing.  Returns one list of InterJointStepReport per step; the frame's squared error after a step is before +
        steps[0].d_sse + steps[1].d_sse exactly.  `roles` must name both roles.  The evaluator keeps one RdoqStep, and the links
        stay: a later alternating descent on this evaluator works as before, because the frozen role's mask is 0 and a slot that
        offers no candidate leaves its partner's step what it would be unlinked."""
        n = len(self._frames)
        order = [_role(r) for r in roles]
        if not order:
            raise ValueError("no role may move")
        if joint and set(order) != {0, 1}:
            raise ValueError("a joint descent moves both roles")
        check_lambda(lmbda, min_gain)
        if n == 0:
            return []
        st = torch.cuda.current_stream(self.device).cuda_stream
        if self._rdoq is None:
            self._rdoq = RdoqStep(self.device)
        for s in range(len(self._rdoq), 2 * n):
            f = self._frames[s // 2]
            self._rdoq.add(f.archs[s % 2], self._fdt(f), f.caller_ptrs[s % 2])
        if joint:
            for k in range(self._n_linked, n):
                self._rdoq.link(2 * k + 1, 2 * k)
            self._n_linked = n
        cycle = [(0, 1)] if joint else [(r,) for r in order]  # the roles that move, step after step
        fixed = []  # per slot: kD, kR, the mask of a step in which its role moves, its grids
        for s in range(2 * n):
            n_grids = int(self._frames[s // 2].archs[s % 2].n_grids)
            g_ok = grids.get(ROLES[s % 2], grids.get(s % 2)) if isinstance(grids, dict) else grids
            fixed.append((*self.move_scales(s // 2, lmbda), grid_mask(n_grids, g_ok), range(n_grids)))
        reports, idle = [], 0
        for step in range(int(max_steps)):
            moving = cycle[step % len(cycle)]
            before = self.evaluate(lmbda, rate_deltas=True, distortion_deltas=True, roles=moving)
            slots = []
            for s, (kD, kR, mask, gs) in enumerate(fixed):  # a role that does not move: mask 0, no distortion maps
                moves = s % 2 in moving
                slots.append(SlotMaps(kD, kR, mask if moves else 0,
                                      [dev_ptr(self._dd[s % 2].delta_map(s // 2, g)) for g in gs] if moves else None,
                                      [dev_ptr(self._enc.delta_map(s, g)) for g in gs]))
            results = run_step(self._rdoq, st, slots, min_gain, rounds)
            if joint:
                reports.append([InterJointStepReport(b, (results[2 * k], results[2 * k + 1])) for k, b in enumerate(before)])
            else:
                reports.append([InterStepReport(b, ROLES[moving[0]], results[2 * k + moving[0]]) for k, b in enumerate(before)])
            idle = 0 if any(r.n_moves for s, r in enumerate(results) if s % 2 in moving) else idle + 1
            if idle >= len(cycle):  # every role set of the cycle has had a step since the last move
                break
        return reports

    def step_moves(self, frame: int, role, grid: int):
        """After descend(): the last step's move (-1, 0, +1) at every latent of the grid (device, int8 [h][w])."""
        if self._rdoq is None:
            raise RuntimeError("no descend() has run")
        return self._rdoq.moves(2 * int(frame) + _role(role), grid)
