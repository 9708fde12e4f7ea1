"""NetworkQuantiser: float network parameters -> the cheapest integers a decoder can be given at this lambda.

The counterpart of the reference's nnquant/quantizemodel.py (quantize_model): per module (ARM, IFCE, upsampling, synthesis) a
search over every (weight step, bias step) pair of the header's tables, the other modules held at their current choice.  The
reference runs its whole test pass once per pair and prices the FLOAT rate estimate and the FLOAT synthesis output; here every
candidate is a decodable integer network, priced by rd.rd_cost from the decoder's own integer ARM (the rate meter) and its own
integer planes (the given-latents float path and the quality meter), a chunk of candidates per launch, all over ONE set of
device latents.  Only the meter that a module can change is run: an ARM / IFCE candidate keeps the base's planes, an upsampling
/ synthesis candidate keeps the base's latent bits.

Differences from the reference, stated: the cost (rd.py's docstring); every group starts at its FINEST step, because a module
that has not been searched yet cannot stay float in a decodable network; each candidate carries its own optimal Exp-Golomb
orders (counted exactly, ties to the smaller order) and its own payload size; ties of the cost go to fewer payload bytes, then
the coarser weight step, then the coarser bias step.

The selection (order of the modules, tie-breaks, sweeps, infeasible cells) is `search_steps`, a pure function over a pricing
callable, so it is testable without a device.  Intra frames only; the two cool-chics of a P / B frame: nnquant_inter.py.

With `dependents` a candidate is also priced through the P / B frames that predict from the frame: the planes a
plane-moving candidate (upsampling, synthesis) decodes to become reference items of ONE InterScore that holds every dependent, one
run per chunk, and the cost of a cell is rd.cost_with_dependents.  Depth one: the dependents' own dependents are not followed."""
import itertools
import time
from typing import TYPE_CHECKING, Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import writer
from ._lib import CcdError, CCHeader

if TYPE_CHECKING:
    from .rd import Candidate

# the library's ways of refusing a NETWORK (CCD_ERR_VALUE, CCD_ERR_INVALID_DATA, CCD_ERR_UNSUPPORTED): such a candidate is
# infeasible.  Every other error (out of memory, HIP, a wrong argument) says nothing about the candidate and is raised.
REFUSALS = (-2, -3, -4)
MODULES = (("arm", 0, 1), ("ifce", 2, 3), ("upsampling", 4, 5), ("synthesis", 6, 7))  # (name, weight group, bias group)


class Cell(NamedTuple):
    """One (weight step, bias step) pair of a module's table.  An infeasible cell has no prices (nan) and is never chosen."""
    q_w: int
    q_b: int
    feasible: bool
    n_bytes_nn: int
    mse: float
    bits: float
    cost: float


class ModuleTable(NamedTuple):
    sweep: int
    module: str
    cells: List[Cell]       # weight steps finest first, bias steps finest first inside
    chosen: Optional[int]   # index into cells; None: no cell was feasible and the module kept its steps


class Pricing(NamedTuple):
    """How one table was priced (NetworkQuantiser's bookkeeping, for tools/rd_bench.py; the selection knows nothing of it)."""
    seconds: float          # wall time of the whole table
    build_seconds: float    # of which: building the candidates on the host (quantise, Exp-Golomb orders, payload)
    chunk: int              # candidates in flight per launch


class QuantisedNetwork(NamedTuple):
    header: CCHeader        # arch with nn_q_step_log2, nn_expgol_cnt, nn_n_bytes and nn_n_bit_pad set
    bytes_nn: bytes
    values: np.ndarray      # int32, stream order
    candidate: "Candidate"  # of the result, from RdEvaluator.evaluate
    tables: List[ModuleTable]
    pricing: List[Pricing]  # one per table
    dependents: tuple = ()  # search(dependents=...): (sse[3], n[3]) of every dependent against the result's planes, in their order


class Dependent(NamedTuple):
    """A P / B frame that predicts from the searched frame (NetworkQuantiser.search(dependents=...)): the frame as
    InterScore.add_frame takes it, with the searched frame as its reference `which`."""
    frame_type: int                 # 1 P, 2 B
    which: int                      # 0 / 1: which of the dependent's references the searched frame is
    residue_ptr: int                # device f32 [4 | 5][h][w]: the dependent's base residue output
    motion_ptr: int                 # device f32 [2 | 4][h][w]: its base motion output
    other_ref_ptrs: Optional[Sequence[int]]  # B frames: the device integer planes of the OTHER reference
    global_flow: Sequence[int]
    warp_filter_size: int
    source: object                  # the dependent's FrameData
    owner: object = None            # keeps the device memory behind the pointers alive


def module_cells(module: int):
    """[(q_w, q_b)] of a module's table in table order."""
    _, gw, gb = MODULES[module]
    return list(itertools.product(writer.q_step_range(gw), writer.q_step_range(gb)))


def choose(cells: Sequence[Cell]) -> Optional[int]:
    """Lowest cost; ties: fewer payload bytes, then the coarser weight step, then the coarser bias step.  None: nothing feasible."""
    best = None
    for i, c in enumerate(cells):
        if not c.feasible:
            continue
        key = (c.cost, c.n_bytes_nn, -c.q_w, -c.q_b)
        if best is None or key < best[0]:
            best = (key, i)
    return None if best is None else best[1]


def _sweep(price, has_ifce: Sequence[bool], sweeps: int, chosen, labels: Sequence[str]):
    """The selection over len(has_ifce) networks: every group starts at its finest step; a sweep visits network 0's ARM, IFCE
    (skipped where has_ifce[network] is false), upsampling and synthesis, then the next network's, and gives each the choose() of
    price(network, module, steps [n][8]) - all pairs of its table, everything else as it stands.  A module without a feasible cell
    keeps its steps.  Sweeps repeat, up to `sweeps`, until one changes nothing.  `chosen(network, module, cell index)` is told
    every choice.  Returns (steps [n][8], [(sweep, network, module, cells, chosen)]); labels[network] is for the error's text."""
    steps = [[writer.q_step_range(g)[0] for g in range(8)] for _ in has_ifce]
    tables = []
    for sweep in range(max(int(sweeps), 1)):
        changed = False
        for net, own in enumerate(steps):
            for m, (name, gw, gb) in enumerate(MODULES):
                if name == "ifce" and not has_ifce[net]:
                    continue
                cells = list(price(net, m, [list(s) for s in steps]))
                if [(c.q_w, c.q_b) for c in cells] != module_cells(m):
                    raise ValueError(f"the {labels[net]}{name} table is not the {len(module_cells(m))} pairs of its groups' steps")
                k = choose(cells)
                tables.append((sweep, net, name, cells, k))
                if k is None:
                    continue
                if chosen is not None:
                    chosen(net, m, k)
                if (cells[k].q_w, cells[k].q_b) != (own[gw], own[gb]):
                    own[gw], own[gb] = cells[k].q_w, cells[k].q_b
                    changed = True
        if not changed:
            break
    return steps, tables


def search_steps(price: Callable[[int, List[int]], Sequence[Cell]], has_ifce: bool, sweeps: int = 1,
                 chosen: Optional[Callable[[int, int], None]] = None):
    """The selection (_sweep) over one network: price(module, steps [8]), chosen(module, cell index) -> (steps [8], [ModuleTable])."""
    steps, tables = _sweep(lambda _, m, steps: price(m, steps[0]), [has_ifce], sweeps,
                           None if chosen is None else lambda _, m, k: chosen(m, k), [""])
    return steps[0], [ModuleTable(sweep, name, cells, k) for sweep, _, name, cells, k in tables]


class _Network(NamedTuple):
    header: CCHeader
    bytes_nn: bytes
    values: np.ndarray
    feasible: bool = True   # False: encodable, but beyond the header's nn_n_bytes or, when asked for, outside the fast path


def refused(call, *args, **kwargs):
    """(result of call(...), False), or (None, True) where the library refuses the network (REFUSALS); any other error is raised."""
    try:
        return call(*args, **kwargs), False
    except CcdError as e:
        if e.code not in REFUSALS:
            raise
        return None, True


def add_networks(add, nets: Sequence[tuple], *args, **kwargs) -> List[Tuple[int, int]]:
    """add(header, bytes_nn, *args, **kwargs) of every network: [(index into nets, slot)] of those the library does not refuse."""
    slots = []
    for i, net in enumerate(nets):
        s, no = refused(add, net[0], net[1], *args, **kwargs)
        if not no:
            slots.append((i, s))
    return slots


def network_rates(device: int, nets: Sequence[Tuple[CCHeader, bytes]], latent_ptrs: Sequence[int], owner=None, stream: int = 0,
                  raise_status: bool = False) -> list:
    """(total_bits, n_bytes_header) per (header, bytes_nn) over the device latents, None where the library refuses the network:
    the rate meter alone, one EncodeBatch, one measure and one wait.  raise_status: a slot the meter leaves with a negative
    status (a latent outside the alphabet) raises it."""
    from .encoder import EncodeBatch

    out = [None] * len(nets)
    with EncodeBatch(device) as enc:
        slots = add_networks(enc.add_device, nets, latent_ptrs, owner=owner)
        if slots:
            enc.measure(stream)
            enc.wait(stream)
            for i, s in slots:
                r = enc.rate(s)
                if raise_status and r.status < 0:
                    raise CcdError(r.status, "ccd_enc_slot_rate")
                out[i] = (r.total_bits, r.n_bytes_header)
    return out


def build_network(arch: CCHeader, float_values: np.ndarray, steps: Sequence[int], fast_path_only: bool = False) -> Optional[_Network]:
    """The integer network of `float_values` at `steps` with its best Exp-Golomb orders; None where the quantiser refuses a
    value or a step (CCD_ERR_VALUE).  Not `feasible`: a payload beyond the header's 14-bit nn_n_bytes (the header writer does
    not refuse it, it writes the low 14 bits), or, with fast_path_only, an ARM outside the pipelined entropy kernel's envelope
    or a network that check refuses.  Errors that are no refusal of the network (REFUSALS) are raised."""
    h = CCHeader.from_buffer_copy(bytes(arch))
    values, no = refused(writer.quantise_network, h, float_values, steps)
    if no:
        return None
    orders, _ = writer.best_expgol(h, values)
    for g in range(8):
        h.nn_q_step_log2[g], h.nn_expgol_cnt[g] = int(steps[g]), orders[g]
    nn = writer.encode_network(h, values)
    feasible = len(nn) <= writer.MAX_NN_BYTES
    if feasible and fast_path_only:
        fits, no = refused(writer.fits_fast_path, writer.cc_header_bytes(h), nn)
        feasible = bool(fits) and not no
    return _Network(h, nn, values, feasible)


def float_network(arch: CCHeader, float_values, source, name: str = ""):
    """(float32 parameters in stream order, writer.network_layout(arch)) of a network to search, checked against both."""
    if tuple(arch.img_size) != tuple(source.img_size):
        raise ValueError(f"the {name + ' ' if name else ''}architecture is {arch.img_size[0]}x{arch.img_size[1]}, the source "
                         f"{source.img_size[0]}x{source.img_size[1]}")
    x = np.ascontiguousarray(float_values, dtype=np.float32).ravel()
    layout = writer.network_layout(arch)
    if x.size != sum(layout):
        raise ValueError("%s%d parameters, the layout wants %d" % (name + ": " if name else "", x.size, sum(layout)))
    return x, layout


def module_candidates(arch: CCHeader, float_values: np.ndarray, steps: Sequence[int], module: int, fast_path_only: bool = False):
    """(module_cells(module), the build_network of every cell): the module at each pair of its table, the others at `steps`."""
    _, gw, gb = MODULES[module]
    pairs = module_cells(module)
    nets = []
    for q_w, q_b in pairs:
        s = list(steps)
        s[gw], s[gb] = q_w, q_b
        nets.append(build_network(arch, float_values, s, fast_path_only))
    return pairs, nets


def chunk_size(max_in_flight_bytes: int, arch: CCHeader, module: int, n_dependents: int = 0) -> int:
    """Candidates per launch: max_in_flight_bytes over the slot_bytes estimate, at least one."""
    return max(1, int(max_in_flight_bytes) // NetworkQuantiser.slot_bytes(arch, module, n_dependents))


def table_chunk(max_in_flight_bytes: int, arch: CCHeader, need_rate: bool, need_planes: bool, n_dependents: int = 0) -> int:
    """Candidates per launch of a table: the smaller chunk_size of the meters that run for it."""
    return min(chunk_size(max_in_flight_bytes, arch, 0) if need_rate else 1 << 30,
               chunk_size(max_in_flight_bytes, arch, 2, n_dependents) if need_planes else 1 << 30)


def table_cells(pairs: Sequence[Tuple[int, int]], nets: Sequence[Optional[_Network]], priced: dict, cost) -> List[Cell]:
    """The table's cells: cell i is feasible where `priced` has it, at (mse, bits, cost) = cost(payload bytes, priced[i])."""
    cells = []
    for i, (q_w, q_b) in enumerate(pairs):
        n_nn = len(nets[i].bytes_nn) if nets[i] is not None else -1
        if i in priced:
            cells.append(Cell(q_w, q_b, True, n_nn, *cost(n_nn, priced[i])))
        else:
            cells.append(Cell(q_w, q_b, False, n_nn, float("nan"), float("nan"), float("nan")))
    return cells


def check_dependents(source, dependents) -> list:
    """The Dependent list of a search over `source`; ValueError for one of another size, format or bit depth, a frame type that is
    not P / B, a reference index the frame type does not have, a B frame without its other reference."""
    from .quality import scored_frame_type

    deps = list(dependents or ())
    own = (tuple(source.img_size), scored_frame_type(source), int(source.bitdepth))
    for k, d in enumerate(deps):
        if (tuple(d.source.img_size), scored_frame_type(d.source), int(d.source.bitdepth)) != own:
            raise ValueError(f"dependent {k} is {d.source.img_size[0]}x{d.source.img_size[1]} {d.source.frame_data_type} at "
                             f"{d.source.bitdepth} bits, the frame {source.img_size[0]}x{source.img_size[1]} {source.frame_data_type} "
                             f"at {source.bitdepth} bits")
        if int(d.frame_type) not in (1, 2) or int(d.which) not in (0, 1) or (int(d.frame_type) == 1 and int(d.which) != 0):
            raise ValueError(f"dependent {k}: frame_type {d.frame_type} with the frame as its reference {d.which}")
        if int(d.frame_type) == 2 and d.other_ref_ptrs is None:
            raise ValueError(f"dependent {k} is a B frame without its other reference's planes")
    return deps


class NetworkQuantiser:
    """search(): the q-step search of one intra frame's networks on one MI355X."""

    def __init__(self, device: int = 0, max_in_flight_bytes: int = 4 << 30):
        """max_in_flight_bytes: the budget the chunks are sized for with slot_bytes' estimate; not a hard limit."""
        self.device = int(device)
        self.max_in_flight_bytes = int(max_in_flight_bytes)

    @staticmethod
    def slot_bytes(arch: CCHeader, module: int, n_dependents: int = 0) -> int:
        """Device bytes one candidate of this module is COUNTED with when chunks are sized - an estimate from the architecture,
        not what the handles allocate (their tables, partial sums and the block pool's rounding come on top; measured 17 %
        above the budget on a 1080p frame): a rate-meter slot (ARM, IFCE: the encoder's pair and payload
        buffers) or a given-latents decode slot (latents, dense stack, float output, planes).  n_dependents: a plane-moving
        candidate is also a reference item of every dependent, 12 bytes per pixel each (its planes as the warp reads them)."""
        n_sym, px = int(arch.n_symbols), int(arch.img_size[0]) * int(arch.img_size[1])
        if module < 2:
            return 16 * n_sym + (64 << 10)
        return n_sym + px * (4 * int(arch.input_feature_synthesis) + 4 * int(arch.out_channels) + 6 + 12 * int(n_dependents)) + (64 << 10)

    def chunk_size(self, arch: CCHeader, module: int, n_dependents: int = 0) -> int:
        """Candidates per launch: max_in_flight_bytes over the slot_bytes estimate, at least one."""
        return chunk_size(self.max_in_flight_bytes, arch, module, n_dependents)

    def search(self, arch: CCHeader, float_values: np.ndarray, latent_ptrs: Sequence[int], source, lmbda: float, sweeps: int = 1,
               fast_path_only: bool = False, owner=None, dependents: Optional[Sequence[Dependent]] = None) -> QuantisedNetwork:
        """arch: the architecture (the transmitted fields but the networks' are read); float_values: float32 parameters in
        stream order (writer.network_layout); latent_ptrs: device latents as RdEvaluator.add takes them (int8 [h][w] per grid,
        kept alive by `owner`); source: the FrameData the planes are scored against.  dependents: the P / B frames that predict
        from this frame (Dependent; same size, format and bit depth, else ValueError): every cell's cost becomes
        rd.cost_with_dependents - an upsampling / synthesis candidate's planes are scored as the dependents' reference, an ARM /
        IFCE candidate keeps the current network's dependent term as it keeps its sse.  None: nothing changes."""
        import torch

        from .quality import _frame_planes, scored_frame_type
        from .rdoq import check_lambda

        check_lambda(lmbda)
        fdt = scored_frame_type(source)
        deps = check_dependents(source, dependents)
        x, layout = float_network(arch, float_values, source)
        ptrs = [int(p) for p in latent_ptrs]
        dev = torch.device(f"cuda:{self.device}")
        st = torch.cuda.current_stream(self.device).cuda_stream
        src_planes = _frame_planes(source, dev)
        n_samples = [int(t.numel()) for t in src_planes]
        score = None
        if deps:
            from .iscore import InterScore

            # every dependent once; the reference the candidates replace is never read through the frame (the source planes
            # stand in for it), a B frame's other reference is warped once per run by the base pair and kept
            score = InterScore(self.device)
            own = [t.data_ptr() for t in src_planes]
            for d in deps:
                d_src = _frame_planes(d.source, dev)
                refs = [own, own]
                if int(d.frame_type) == 2:
                    refs[1 - int(d.which)] = [int(p) for p in d.other_ref_ptrs]
                score.add_frame(int(d.frame_type), int(source.img_size[0]), int(source.img_size[1]), int(source.bitdepth), fdt, int(d.residue_ptr),
                                int(d.motion_ptr), refs[0], refs[1] if int(d.frame_type) == 2 else None, [t.data_ptr() for t in d_src],
                                d.global_flow, int(d.warp_filter_size), owner=(d.owner, d_src, src_planes))
        try:
            return self._search(arch, x, layout, ptrs, source, lmbda, sweeps, fast_path_only, owner, deps, score, src_planes, n_samples, fdt, dev, st)
        finally:
            if score is not None:
                score.close()

    def _search(self, arch, x, layout, ptrs, source, lmbda, sweeps, fast_path_only, owner, deps, score, src_planes, n_samples, fdt, dev, st):
        import torch

        from .batch import DecodeBatch
        from .quality import QualityMeter
        from .rd import RdEvaluator, cost_with_dependents, rd_cost

        def full(net: _Network):
            with RdEvaluator(self.device) as ev:
                ev.add(net.header, net.bytes_nn, ptrs, source, owner=owner)
                return ev.evaluate(lmbda)[0]

        # what the meter that a module does NOT run would say: the current network's; None until a network has been priced
        state = {"total_bits": None, "sse": None, "n_bytes_header": None, "dep": None}
        pricing: List[Pricing] = []
        priced: dict = {}   # of the table being chosen from: cell index -> (total_bits, sse, n_bytes_header, dependents' (sse, n))

        def rates(nets: List[_Network]):
            return network_rates(self.device, [(net.header, net.bytes_nn) for net in nets], ptrs, owner, st)

        def errors(nets: List[_Network]):
            """(sse per plane, the dependents' (sse, n) or None) per network, None where the library refuses it: the float path
            over the given latents and the quality meter alone, and the networks' planes as reference items of every dependent."""
            out = [None] * len(nets)
            with DecodeBatch(self.device) as dec, QualityMeter(self.device) as meter:
                slots = add_networks(dec.add_latents_device, nets, ptrs, source.bitdepth, fdt, owner=owner)
                if slots:
                    dec.run(st)
                    decoded = [[torch.as_tensor(dec.plane_device(s, p), device=dev) for p in range(3)] for _, s in slots]
                    meter.score_planes_async(decoded, [src_planes] * len(slots), [source.bitdepth] * len(slots), False, stream=st)
                    items = []
                    if score is not None:  # same stream: behind the float path that writes the planes
                        for planes in decoded:
                            pp = [t.data_ptr() for t in planes]
                            items.append([score.add_refs(k, pp if int(d.which) == 0 else None, pp if int(d.which) == 1 else None)
                                          for k, d in enumerate(deps)])
                        score.run(st)
                    res = meter.finish()
                    dec.wait(st)
                    if score is not None:
                        score.wait(st)
                    for j, ((i, _), r) in enumerate(zip(slots, res)):
                        out[i] = (tuple(int(v) for v in r.sse), tuple(score.sse(it) for it in items[j]) if score is not None else None)
                    if score is not None:
                        score.clear_items()
            return out

        start = build_network(arch, x, [writer.q_step_range(g)[0] for g in range(8)], fast_path_only)
        if start is not None and start.feasible:
            c, no = refused(full, start)
            if not no:
                state.update(total_bits=c.rate.total_bits, sse=tuple(c.quality.sse), n_bytes_header=c.rate.n_bytes_header)
                if score is not None:
                    state.update(dep=errors([start])[0][1])

        def price(m: int, steps: List[int]) -> List[Cell]:
            t0 = time.perf_counter()
            pairs, nets = module_candidates(arch, x, steps, m, fast_path_only)
            t_built = time.perf_counter()
            need_rate = m < 2 or state["total_bits"] is None
            need_planes = m >= 2 or state["sse"] is None
            chunk = table_chunk(self.max_in_flight_bytes, arch, need_rate, need_planes, len(deps))
            live = [i for i, n in enumerate(nets) if n is not None and n.feasible]
            priced.clear()
            for at in range(0, len(live), chunk):
                part = live[at:at + chunk]
                r = rates([nets[i] for i in part]) if need_rate else [(state["total_bits"], state["n_bytes_header"])] * len(part)
                e = errors([nets[i] for i in part]) if need_planes else [(state["sse"], state["dep"])] * len(part)
                for i, ri, ei in zip(part, r, e):
                    if ri is not None and ei is not None:
                        priced[i] = (ri[0], ei[0], ri[1], ei[1])

            def cost(n_nn: int, p):
                total_bits, sse, n_hdr, dep = p
                own = rd_cost(sse, n_samples, source.bitdepth, total_bits, n_nn, n_hdr, source.n_pixels, lmbda)
                if score is None:
                    return own
                return own[0], own[1], cost_with_dependents(own, [(d_sse, d_n, source.bitdepth) for d_sse, d_n in dep])

            cells = table_cells(pairs, nets, priced, cost)
            pricing.append(Pricing(time.perf_counter() - t0, t_built - t0, chunk))
            return cells

        def chosen(m: int, k: int) -> None:
            total_bits, sse, n_hdr, dep = priced[k]
            state.update(total_bits=total_bits, sse=sse, n_bytes_header=n_hdr, dep=dep)

        steps, tables = search_steps(price, layout[2] > 0, sweeps, chosen)
        net = build_network(arch, x, steps, fast_path_only)
        if net is None or not net.feasible:
            raise ValueError("no feasible network was found: every candidate of the module that holds the start back is infeasible "
                             "(a payload beyond 16 383 bytes, a refused value or, with fast_path_only, an ARM outside the fast path)")
        result = full(net)
        return QuantisedNetwork(net.header, net.bytes_nn, net.values, result, tables, pricing, errors([net])[0][1] if score is not None else ())
