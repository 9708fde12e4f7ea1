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
from ._lib import CCHeader
from .nnquant import MODULES, Cell, Pricing, _Network, build_network, choose, module_cells, network_rates, refused

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
    """nnquant.search_steps over two networks: every group of both starts at its finest step; a sweep visits the residue
    cool-chic's ARM, IFCE (skipped where has_ifce[role] is false), upsampling and synthesis, then the motion cool-chic's, and gives
    each the choose() of price(role, module, current steps [2][8]) - all pairs of the module's table, everything else as it
    stands.  A module without a feasible cell keeps its steps.  Sweeps repeat, up to `sweeps`, until one changes nothing.
    `chosen(role, module, cell index)` is told every choice.  Returns (steps [2][8], [InterModuleTable])."""
    steps = [[writer.q_step_range(g)[0] for g in range(8)] for _ in range(2)]
    tables: List[InterModuleTable] = []
    for sweep in range(max(int(sweeps), 1)):
        changed = False
        for role in range(2):
            for m, (name, gw, gb) in enumerate(MODULES):
                if name == "ifce" and not has_ifce[role]:
                    continue
                cells = list(price(role, m, [list(s) for s in steps]))
                if [(c.q_w, c.q_b) for c in cells] != module_cells(m):
                    raise ValueError(f"the {ROLES[role]} {name} table is not the {len(module_cells(m))} pairs of its groups' steps")
                k = choose(cells)
                tables.append(InterModuleTable(sweep, role, name, cells, k))
                if k is None:
                    continue
                if chosen is not None:
                    chosen(role, m, k)
                if (cells[k].q_w, cells[k].q_b) != (steps[role][gw], steps[role][gb]):
                    steps[role][gw], steps[role][gb] = cells[k].q_w, cells[k].q_b
                    changed = True
        if not changed:
            break
    return steps, tables


class InterNetworkQuantiser:
    """search(): the q-step search of the two cool-chics of one P / B frame on one MI355X."""

    def __init__(self, device: int = 0, max_in_flight_bytes: int = 4 << 30):
        """max_in_flight_bytes: the budget the chunks are sized for with NetworkQuantiser.slot_bytes' estimate; not a hard limit."""
        self.device = int(device)
        self.max_in_flight_bytes = int(max_in_flight_bytes)

    def chunk_size(self, arch: CCHeader, module: int) -> int:
        """Candidates per launch: max_in_flight_bytes over NetworkQuantiser.slot_bytes, at least one."""
        from .nnquant import NetworkQuantiser

        return max(1, self.max_in_flight_bytes // NetworkQuantiser.slot_bytes(arch, module))

    def search(self, frame_type, residue, motion, references: Sequence, global_flow: Sequence[int], warp_filter_size: int, source,
               lmbda: float, sweeps: int = 1, fast_path_only: bool = False, owner=None) -> QuantisedInterNetworks:
        """frame_type: 'P' / 'B' (1 / 2).  residue, motion: (arch, float_values, latent_ptrs) - the architecture (the transmitted
        fields but the networks' are read), float32 parameters in stream order (writer.network_layout), device latents (int8
        [h][w] per grid, kept alive by `owner`).  references, global_flow, warp_filter_size, source: as InterRdEvaluator.add
        takes them."""
        import torch

        from .batch import FRAME_DATA_TYPES, DecodeBatch
        from .io import FrameData
        from .iscore import InterScore
        from .quality import _frame_planes
        from .rd import rd_cost
        from .rd_inter import InterRdEvaluator

        ft = {"P": 1, "B": 2}.get(frame_type, frame_type)
        if ft not in (1, 2):
            raise ValueError(f"frame_type must be 'P' / 'B' (1 / 2), not {frame_type!r}")
        if not np.isfinite(float(lmbda)) or float(lmbda) < 0.0:
            raise ValueError("lmbda must be finite and not negative")
        if source.frame_data_type not in ("rgb", "yuv420", "yuv444"):
            raise ValueError(f"cannot score a {source.frame_data_type} frame")
        if len(references) < ft:
            raise ValueError(f"a {'PB'[ft - 1]} frame needs {ft} reference frame(s)")
        archs, xs, ptrs, layouts = [], [], [], []
        for role, (arch, float_values, latent_ptrs) in enumerate((residue, motion)):
            if tuple(arch.img_size) != tuple(source.img_size):
                raise ValueError(f"the {ROLES[role]} architecture is {arch.img_size[0]}x{arch.img_size[1]}, the source "
                                 f"{source.img_size[0]}x{source.img_size[1]}")
            x = np.ascontiguousarray(float_values, dtype=np.float32).ravel()
            layout = writer.network_layout(arch)
            if x.size != sum(layout):
                raise ValueError("%s: %d parameters, the layout wants %d" % (ROLES[role], x.size, sum(layout)))
            archs.append(arch); xs.append(x); layouts.append(layout); ptrs.append([int(p) for p in latent_ptrs])
        fdt = FRAME_DATA_TYPES.index(source.frame_data_type)
        dev = torch.device(f"cuda:{self.device}")
        st = torch.cuda.current_stream(self.device).cuda_stream
        src = _frame_planes(source, dev)
        refs = [_frame_planes(r, dev) if isinstance(r, FrameData) else [p for p in r] for r in list(references)[:ft]]
        gf = ([int(v) for v in global_flow] + [0, 0, 0, 0])[:4]
        h, w = (int(v) for v in source.img_size)
        bitdepth = int(source.bitdepth)

        def rates(role: int, nets: List[_Network]):
            return network_rates(self.device, [(net.header, net.bytes_nn) for net in nets], ptrs[role], owner, st)

        def decode(role: int, nets: List[_Network], use):
            """The float outputs of the networks over the role's latents: use(dec, [(index into nets, device address)]) runs
            while they are valid; networks the library refuses are left out."""
            with DecodeBatch(self.device) as dec:
                slots = []
                for i, net in enumerate(nets):
                    s, no = refused(dec.add_latents_device, net.header, net.bytes_nn, ptrs[role], 0, 0, owner=owner)
                    if not no:
                        slots.append((i, s))
                if not slots:
                    return None
                dec.run(st)
                out = use(dec, [(i, int(dec.output_device(s).__cuda_array_interface__["data"][0])) for i, s in slots])
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
            _, gw, gb = MODULES[m]
            pairs = module_cells(m)
            arch, other = archs[role], 1 - role
            nets = []
            for q_w, q_b in pairs:
                s = list(steps[role])
                s[gw], s[gb] = q_w, q_b
                nets.append(build_network(arch, xs[role], s, fast_path_only))
            t_built = time.perf_counter()
            need_rate = m < 2 or bits[role] is None
            need_planes = m >= 2 or state["sse"] is None
            chunk = min(self.chunk_size(arch, 0) if need_rate else 1 << 30, self.chunk_size(arch, 2) if need_planes else 1 << 30)
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
            cells = []
            for i, (q_w, q_b) in enumerate(pairs):
                if i not in priced:
                    cells.append(Cell(q_w, q_b, False, len(nets[i].bytes_nn) if nets[i] is not None else -1, float("nan"), float("nan"), float("nan")))
                    continue
                (total_bits, n_hdr), sse, _ = priced[i]
                n_nn = len(nets[i].bytes_nn)
                mse, b, cost = rd_cost(sse, n_samples, bitdepth, total_bits + bits[other][0], n_nn + len(cur[other].bytes_nn),
                                       n_hdr + bits[other][1], source.n_pixels, lmbda)
                cells.append(Cell(q_w, q_b, True, n_nn, mse, b, cost))
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
