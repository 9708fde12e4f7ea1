"""InterNetworkQuantiser: the q-step search of nnquant.NetworkQuantiser for the TWO cool-chics of a P / B frame.

A candidate replaces one module of one cool-chic, the other cool-chic and the other modules held at their current choice.  Its
cost is what InterRdEvaluator.evaluate returns for the pair - rd.rd_cost over the frame's squared error after the reconstruction
and the model bits, network bytes and cool-chic header bytes of both cool-chics - but only the meter the module can change runs:
an ARM / IFCE candidate of a role goes through the rate meter over that role's latents and keeps the frame's squared error and
the partner's bits; an upsampling / synthesis candidate goes through the float path (float output, no planes of its own) and
iscore.InterScore, which reconstructs and scores every candidate of a chunk in one launch, and keeps the bits.

Differences from the reference (nnquant/quantizemodel.py), stated: those of nnquant.py's docstring, and the order - the reference
quantises each cool-chic of a frame on its own against the float output of the other, here the residue cool-chic's four modules
are chosen first against the motion cool-chic at its current (at first: finest) steps, then the motion cool-chic's against the
chosen residue; further sweeps repeat both.

The selection is `search_steps_pair`, a pure function over a pricing callable."""
import time
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import writer
from ._handle import dev_ptr
from ._lib import CCHeader
from .nnquant import (Cell, Pricing, _Network, _sweep, add_networks, build_network, chunk_size, float_network, module_candidates,
                      network_rates, table_cells, table_chunk)

ROLES = ("residue", "motion")


class InterModuleTable(NamedTuple):
    sweep: int
    role: int               # 0 residue, 1 motion
    module: str
    cells: List[Cell]       # weight steps finest first, bias steps finest first inside
    chosen: Optional[int]   # index into cells; None: no cell was feasible and the module kept its steps


class RoleNetwork(NamedTuple):
    header: CCHeader        # arch with nn_q_step_log2, nn_expgol_cnt, nn_n_bytes and nn_n_bit_pad set
    bytes_nn: bytes
    values: np.ndarray      # int32, stream order


class QuantisedInterNetworks(NamedTuple):
    residue: RoleNetwork
    motion: RoleNetwork
    candidate: "object"     # InterCandidate of the result, from InterRdEvaluator.evaluate
    tables: List[InterModuleTable]
    pricing: List[Pricing]  # one per table

    @property
    def roles(self) -> Tuple[RoleNetwork, RoleNetwork]:
        return (self.residue, self.motion)


def search_steps_pair(price: Callable[[int, int, List[List[int]]], Sequence[Cell]], has_ifce: Tuple[bool, bool] = (False, False),
                      sweeps: int = 1, chosen: Optional[Callable[[int, int, int], None]] = None):
    """nnquant.search_steps over two networks (nnquant._sweep): the residue cool-chic's modules, then the motion cool-chic's, each
    given the choose() of price(role, module, current steps [2][8]); `chosen(role, module, cell index)` is told every choice.
    Returns (steps [2][8], [InterModuleTable])."""
    steps, tables = _sweep(price, has_ifce, sweeps, chosen, [r + " " for r in ROLES])
    return steps, [InterModuleTable(*t) for t in tables]


class InterNetworkQuantiser:
    """search(): the q-step search of the two cool-chics of one P / B frame on one MI355X."""

    def __init__(self, device: int = 0, max_in_flight_bytes: int = 4 << 30):
        """max_in_flight_bytes: the budget the chunks are sized for with NetworkQuantiser.slot_bytes' estimate; not a hard limit."""
        self.device = int(device)
        self.max_in_flight_bytes = int(max_in_flight_bytes)

    def chunk_size(self, arch: CCHeader, module: int) -> int:
        """Candidates per launch (nnquant.chunk_size of max_in_flight_bytes)."""
        return chunk_size(self.max_in_flight_bytes, arch, module)

    def search(self, frame_type, residue, motion, references: Sequence, global_flow: Sequence[int], warp_filter_size: int, source,
               lmbda: float, sweeps: int = 1, fast_path_only: bool = False, owner=None) -> QuantisedInterNetworks:
        """frame_type: 'P' / 'B' (1 / 2).  residue, motion: (arch, float_values, latent_ptrs) - the architecture (the transmitted
        fields but the networks' are read), float32 parameters in stream order (writer.network_layout), device latents (int8
        [h][w] per grid, kept alive by `owner`).  references, global_flow, warp_filter_size, source: as InterRdEvaluator.add
        takes them."""
        import torch

        from .batch import DecodeBatch
        from .iscore import InterScore
        from .quality import _frame_planes, scored_frame_type
        from .rd import rd_cost
        from .rd_inter import InterRdEvaluator, inter_frame_type, padded_global_flow, reference_planes
        from .rdoq import check_lambda

        ft = inter_frame_type(frame_type)
        check_lambda(lmbda)
        fdt = scored_frame_type(source)
        dev = torch.device(f"cuda:{self.device}")
        refs = reference_planes(ft, references, dev)
        archs, xs, ptrs, layouts = [], [], [], []
        for role, (arch, float_values, latent_ptrs) in enumerate((residue, motion)):
            x, layout = float_network(arch, float_values, source, ROLES[role])
            archs.append(arch); xs.append(x); layouts.append(layout); ptrs.append([int(p) for p in latent_ptrs])
        st = torch.cuda.current_stream(self.device).cuda_stream
        src = _frame_planes(source, dev)
        gf = padded_global_flow(global_flow)
        h, w = (int(v) for v in source.img_size)
        bitdepth = int(source.bitdepth)

        def rates(role: int, nets: List[_Network]):
            return network_rates(self.device, [(net.header, net.bytes_nn) for net in nets], ptrs[role], owner, st)

        def decode(role: int, nets: List[_Network], use):
            """The float outputs of the networks over the role's latents: use(dec, [(index into nets, device address)]) runs
            while they are valid; networks the library refuses are left out."""
            with DecodeBatch(self.device) as dec:
                slots = add_networks(dec.add_latents_device, nets, ptrs[role], 0, 0, owner=owner)
                if not slots:
                    return None
                dec.run(st)
                out = use(dec, [(i, dev_ptr(dec.output_device(s))) for i, s in slots])
                dec.wait(st)  # a refused device latent raises here (CCD_ERR_VALUE)
                return out

        def output_of(role: int, net: _Network):
            """The role's float output under `net`, cloned; None where the library refuses the network."""
            def clone(dec, outs):
                t = torch.as_tensor(dec.output_device(0), device=dev)[0].clone()
                torch.cuda.current_stream(self.device).synchronize()
                return t
            return decode(role, [net], clone)

        # what the pair is now: per role the network (None: nothing decodable yet), its (total_bits, n_bytes_header) and its
        # float output; the frame's squared error under both (None until a pair has been scored)
        cur: List[Optional[_Network]] = [None, None]
        bits: List[Optional[tuple]] = [None, None]
        out: List[Optional[torch.Tensor]] = [None, None]
        state = {"sse": None}
        n_samples = [int(t.numel()) for t in src]

        def add_frame(score, residue_out, motion_out):
            return score.add_frame(ft, h, w, bitdepth, fdt, residue_out.data_ptr(), motion_out.data_ptr(), [t.data_ptr() for t in refs[0]],
                                   [t.data_ptr() for t in refs[1]] if ft == 2 else None, [t.data_ptr() for t in src], gf,
                                   int(warp_filter_size), owner=(residue_out, motion_out, refs, src))

        for role in range(2):
            start = build_network(archs[role], xs[role], [writer.q_step_range(g)[0] for g in range(8)], fast_path_only)
            if start is None or not start.feasible:
                continue
            r = rates(role, [start])[0]
            o = output_of(role, start) if r is not None else None
            if r is not None and o is not None:
                cur[role], bits[role], out[role] = start, r, o
        if cur[0] is not None and cur[1] is not None:
            with InterScore(self.device) as score:
                add_frame(score, out[0], out[1])
                score.run(st)
                score.wait(st)
                state["sse"] = score.frame_sse(0)[0]
        pricing: List[Pricing] = []
        priced: dict = {}   # of the table being chosen from: cell index -> ((total_bits, n_bytes_header), sse, network)

        def errors(role: int, nets: List[_Network], score) -> list:
            """sse per plane per network, None where the library refuses it: the float path over the role's latents, then the
            reconstruction and the squared error of every candidate in one InterScore run."""
            res = [None] * len(nets)

            def use(dec, outs):
                score.clear_items()
                items = [(i, score.add(0, role, p)) for i, p in outs]
                score.run(st)
                score.wait(st)
                for i, it in items:
                    res[i] = score.sse(it)[0]

            decode(role, nets, use)
            return res

        def price(role: int, m: int, steps: List[List[int]]) -> List[Cell]:
            t0 = time.perf_counter()
            arch, other = archs[role], 1 - role
            pairs, nets = module_candidates(arch, xs[role], steps[role], m, fast_path_only)
            t_built = time.perf_counter()
            need_rate = m < 2 or bits[role] is None
            need_planes = m >= 2 or state["sse"] is None
            chunk = table_chunk(self.max_in_flight_bytes, arch, need_rate, need_planes)
            # without a decodable partner no pair exists: every cell is infeasible
            live = [i for i, n in enumerate(nets) if n is not None and n.feasible] if cur[other] is not None else []
            priced.clear()
            score = None
            try:
                for at in range(0, len(live), chunk):
                    part = live[at:at + chunk]
                    r = rates(role, [nets[i] for i in part]) if need_rate else [bits[role]] * len(part)
                    if need_planes:
                        if score is None:  # the frame holds the current pair (a role without an output yet: any of its own)
                            own = out[role] if out[role] is not None else None
                            for i in part:
                                if own is not None:
                                    break
                                own = output_of(role, nets[i])
                            if own is None:
                                continue
                            score = InterScore(self.device)
                            add_frame(score, *((own, out[1]) if role == 0 else (out[0], own)))
                        e = errors(role, [nets[i] for i in part], score)
                    else:
                        e = [state["sse"]] * len(part)
                    for i, ri, ei in zip(part, r, e):
                        if ri is not None and ei is not None:
                            priced[i] = (ri, ei, nets[i])
            finally:
                if score is not None:
                    score.close()

            def cost(n_nn: int, p):  # of the pair: the partner's bits and bytes as they stand
                (total_bits, n_hdr), sse, _ = p
                return rd_cost(sse, n_samples, bitdepth, total_bits + bits[other][0], n_nn + len(cur[other].bytes_nn),
                               n_hdr + bits[other][1], source.n_pixels, lmbda)

            cells = table_cells(pairs, nets, priced, cost)
            pricing.append(Pricing(time.perf_counter() - t0, t_built - t0, chunk))
            return cells

        def chosen(role: int, m: int, k: int) -> None:
            r, sse, net = priced[k]
            if m >= 2 or out[role] is None:  # the role's output changes with its upsampling / synthesis (or was not known yet)
                out[role] = output_of(role, net)
            cur[role], bits[role] = net, r
            state["sse"] = sse

        has_ifce = (layouts[0][2] > 0, layouts[1][2] > 0)
        steps, tables = search_steps_pair(price, has_ifce, sweeps, chosen)
        nets = [build_network(archs[role], xs[role], steps[role], fast_path_only) for role in range(2)]
        if any(n is None or not n.feasible for n in nets) or cur[0] is None or cur[1] is None:
            raise ValueError("no feasible pair of networks was found: every candidate of the module that holds a start back is infeasible "
                             "(a payload beyond 16 383 bytes, a refused value or, with fast_path_only, an ARM outside the fast path)")
        with InterRdEvaluator(self.device) as ev:
            ev.add(ft, (nets[0].header, nets[0].bytes_nn, ptrs[0]), (nets[1].header, nets[1].bytes_nn, ptrs[1]), refs, gf, int(warp_filter_size),
                   source, owner=owner)
            cand = ev.evaluate(lmbda)[0]
        return QuantisedInterNetworks(RoleNetwork(nets[0].header, nets[0].bytes_nn, nets[0].values),
                                      RoleNetwork(nets[1].header, nets[1].bytes_nn, nets[1].values), cand, tables, pricing)
