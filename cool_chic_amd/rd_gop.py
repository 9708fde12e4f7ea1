"""GopDescent: requantisation by descent of intra frames TOGETHER with the residues of the P / B frames that predict from them, on
one MI355X.

The intra frames are the candidates of an rd.RdEvaluator, the P / B frames those of an rd_inter.InterRdEvaluator whose references
are the intra candidates' decoded planes (reference_planes()).  follow() declares which intra candidate is which reference of
which frame; it registers the frame as a dependent of the candidate's distortion deltas (RdEvaluator.add_dependent)
and as a follow of its RDOQ slot (RdoqStep.follow).  One step then

    1. decodes the intra candidates (their planes are what the inter frames predict from),
    2. evaluates the inter frames against those planes, with the deltas of their residue cool-chics,
    3. runs the intra candidates' distortion deltas with their dependents,

hands own, dependent and rate maps to ONE RdoqStep - the intra slots first, then two per inter frame - and runs one step in which
the intra slots and the residue slots move and the motion slots do not (the flows are followed as they are).  The selected moves
are pairwise independent inside every frame and through the flows into the followed frames, so the summed squared error of all
frames changes by exactly the sum of d_sse and dep_sse over the slots.

Depth one only: an intra candidate's moves are followed into the frames that predict from it, not into frames that predict from
those; and references that are themselves P / B frames are not supported here (InterRdEvaluator has no add_dependent) - the C
layer and RdoqStep.follow take them."""
from typing import List, NamedTuple, Optional, Sequence

import torch

from ._handle import dev_ptr
from .batch import FRAME_DATA_TYPES
from .rd import Candidate, RdEvaluator
from .rd_inter import InterCandidate, InterRdEvaluator
from .rdoq import RdoqStep, SlotMaps, StepResult, check_lambda, grid_mask, run_step


class GopSlotReport(NamedTuple):
    """One slot of the step's RdoqStep: an intra candidate (frame = its index, role "intra") or one cool-chic of an inter frame."""
    frame: int
    role: str        # "intra", "residue", "motion"
    d_sse: int       # the change of the slot's OWN frame's squared error
    dep_sse: int     # ... of the frames that predict from it (intra slots with follows; 0 otherwise)
    d_bits: float
    step: StepResult


class GopStepReport(NamedTuple):
    intra: List[Candidate]        # the intra candidates before the step
    inter: List[InterCandidate]   # the inter frames before the step
    slots: List[GopSlotReport]

    @property
    def n_moves(self) -> int:
        return sum(s.step.n_moves for s in self.slots)

    @property
    def d_sse(self) -> int:
        """What the step did to the summed squared error of all frames, exactly."""
        return sum(s.d_sse + s.dep_sse for s in self.slots)


class GopDescent:
    def __init__(self, intra: RdEvaluator, inter: InterRdEvaluator):
        if intra.device != inter.device:
            raise ValueError("both evaluators must be on one device")
        self.intra, self.inter = intra, inter
        self.device = intra.device
        self._rdoq: Optional[RdoqStep] = None
        self._follows: List[tuple] = []   # (intra slot, frame, which), in registration order
        self._n_followed = 0              # ... of them registered with the RdoqStep
        self._n_intra = 0                 # the intra slots the RdoqStep holds: fixed once it exists

    def close(self):
        if self._rdoq is not None:
            self._rdoq.close()
            self._rdoq = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reference_planes(self, intra_slot: int) -> List[torch.Tensor]:
        """The integer device planes candidate `intra_slot` decodes to, rewritten by every step: what to give
        InterRdEvaluator.add as the reference of a frame that predicts from it."""
        return self.intra.planes(intra_slot)

    def follow(self, intra_slot: int, frame: int, which: int) -> None:
        """Intra candidate `intra_slot` is reference `which` of inter frame `frame` (which must have been added with
        reference_planes(intra_slot) in that place)."""
        frame, which, intra_slot = int(frame), int(which), int(intra_slot)
        f = self.inter.frame(frame)
        if not 0 <= which < f.frame_type:
            raise ValueError(f"frame {frame} has {f.frame_type} reference(s)")
        if not 0 <= intra_slot < len(self.intra):
            raise IndexError(f"no intra candidate {intra_slot}")
        want = [t.data_ptr() for t in self.reference_planes(intra_slot)]
        if [t.data_ptr() for t in f.refs[which]] != want:
            raise ValueError("the frame's reference is not reference_planes(intra_slot): the step could not follow its moves")
        other = f.refs[1 - which] if f.frame_type == 2 else None
        self.intra.add_dependent(intra_slot, f.frame_type, which, self.inter.output_ptr(frame, "residue"), self.inter.output_ptr(frame, "motion"),
                                 [t.data_ptr() for t in f.src], None if other is None else [t.data_ptr() for t in other], f.global_flow,
                                 f.warp_filter_size, owner=(self.inter, f.src, other))
        self._follows.append((intra_slot, frame, which))

    def _slots(self):
        """The RdoqStep: the intra candidates' slots first, then residue and motion of every inter frame."""
        n_i, n_f = len(self.intra), len(self.inter)
        if self._rdoq is None:
            self._rdoq = RdoqStep(self.device)
            self._n_intra = n_i
            for s in range(n_i):
                if self.intra.caller_latent_ptrs(s) is None:
                    raise ValueError(f"intra candidate {s} was added from host arrays: a step moves device latents the caller owns")
                self._rdoq.add(self.intra.architecture(s), FRAME_DATA_TYPES.index(self.intra.source(s).frame_data_type),
                               self.intra.caller_latent_ptrs(s))
        if n_i != self._n_intra:
            raise ValueError("intra candidates were added after the first step")
        for s in range(len(self._rdoq) - n_i, 2 * n_f):
            f = self.inter.frame(s // 2)
            self._rdoq.add(f.archs[s % 2], self.inter.frame_data_type_index(s // 2), f.caller_ptrs[s % 2])
        for intra_slot, frame, which in self._follows[self._n_followed:]:
            f = self.inter.frame(frame)
            self._rdoq.follow(intra_slot, f.frame_type, which, self.inter.output_ptr(frame, "motion"), target=n_i + 2 * frame,
                              frozen=n_i + 2 * frame + 1, global_flow=f.global_flow, warp_filter_size=f.warp_filter_size, owner=self.inter)
        self._n_followed = len(self._follows)
        return self._rdoq

    def step(self, lmbda: float, min_gain: float = 0.0, grids: Optional[Sequence[int]] = None, rounds: int = 8) -> GopStepReport:
        """One step as the module's docstring orders it.  `grids`: the grids that may move in the intra and the residue
        cool-chics (all by default; the advice of RdEvaluator.descend about the coarse grids holds)."""
        check_lambda(lmbda, min_gain)
        intra, inter = self.intra, self.inter
        n_i, n_f = len(intra), len(inter)
        rdoq = self._slots()
        st = torch.cuda.current_stream(self.device).cuda_stream
        before_i = intra.evaluate(lmbda, rate_deltas=True)                                              # 1.
        before_f = inter.evaluate(lmbda, rate_deltas=True, distortion_deltas=True, roles=("residue",))  # 2.
        intra.run_distortion_deltas()                                                                   # 3.
        followed = {s for s, _, _ in self._follows}
        slots = []
        for s in range(n_i):
            gs = range(int(intra.architecture(s).n_grids))
            slots.append(SlotMaps(*intra.move_scales(s, lmbda), grid_mask(len(gs), grids),
                                  [dev_ptr(intra.distortion_delta_map(s, g)) for g in gs], [dev_ptr(intra.rate_delta_map(s, g)) for g in gs],
                                  [dev_ptr(intra.dependent_delta_map(s, g)) for g in gs] if s in followed else None))
        for s in range(2 * n_f):  # the residues move; the flows are followed as they are
            k, role = divmod(s, 2)
            gs = range(int(inter.frame(k).archs[role].n_grids))
            slots.append(SlotMaps(*inter.move_scales(k, lmbda), grid_mask(len(gs), grids) if role == 0 else 0,
                                  [dev_ptr(inter.distortion_delta_map(k, "residue", g)) for g in gs] if role == 0 else None,
                                  [dev_ptr(inter.rate_delta_map(k, role, g)) for g in gs]))
        results = run_step(rdoq, st, slots, min_gain, rounds)
        reports = []
        for s, res in enumerate(results):
            frame, role = (s, "intra") if s < n_i else ((s - n_i) // 2, ("residue", "motion")[(s - n_i) % 2])
            reports.append(GopSlotReport(frame, role, res.d_sse, rdoq.dep_sse(s), res.d_bits, res))
        return GopStepReport(before_i, before_f, reports)

    def step_moves(self, frame: int, role: str, grid: int):
        """After step(): the move (-1, 0, +1) the last step applied at every latent of the grid (device, int8 [h][w]); `frame` and
        `role` as GopSlotReport names a slot."""
        if self._rdoq is None:
            raise RuntimeError("no step() has run")
        slot = int(frame) if role == "intra" else self._n_intra + 2 * int(frame) + ("residue", "motion").index(role)
        return self._rdoq.moves(slot, grid)

    def descend(self, lmbda: float, max_steps: int, min_gain: float = 0.0, grids: Optional[Sequence[int]] = None,
                rounds: int = 8) -> List[GopStepReport]:
        """step() until a step moves nothing, `max_steps` steps at the most."""
        reports = []
        for _ in range(int(max_steps)):
            reports.append(self.step(lmbda, min_gain, grids, rounds))
            if reports[-1].n_moves == 0:
                break
        return reports
