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
callable, so it is testable without a device.  Intra frames only; the two cool-chics of a P / B frame: nnquant_inter.py."""
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


def search_steps(price: Callable[[int, List[int]], Sequence[Cell]], has_ifce: bool, sweeps: int = 1,
                 chosen: Optional[Callable[[int, int], None]] = None):
    """The selection: every group starts at its finest step; a sweep visits ARM, IFCE (skipped without features), upsampling
    and synthesis, and gives each the choose() of price(module, current steps) - all pairs of the module's table with the other
    modules as they stand.  A module without a feasible cell keeps its steps.  Sweeps repeat, up to `sweeps`, until one changes
    nothing.  `chosen(module, cell index)` is told every choice.  Returns (steps [8], [ModuleTable])."""
    steps = [writer.q_step_range(g)[0] for g in range(8)]
    tables: List[ModuleTable] = []
    for sweep in range(max(int(sweeps), 1)):
        changed = False
        for m, (name, gw, gb) in enumerate(MODULES):
            if name == "ifce" and not has_ifce:
                continue
            cells = list(price(m, list(steps)))
            if [(c.q_w, c.q_b) for c in cells] != module_cells(m):
                raise ValueError(f"the {name} table is not the {len(module_cells(m))} pairs of its groups' steps")
            k = choose(cells)
            tables.append(ModuleTable(sweep, name, cells, k))
            if k is None:
                continue
            if chosen is not None:
                chosen(m, k)
            if (cells[k].q_w, cells[k].q_b) != (steps[gw], steps[gb]):
                steps[gw], steps[gb] = cells[k].q_w, cells[k].q_b
                changed = True
        if not changed:
            break
    return steps, tables


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


def network_rates(device: int, nets: Sequence[Tuple[CCHeader, bytes]], latent_ptrs: Sequence[int], owner=None, stream: int = 0,
                  raise_status: bool = False) -> list:
    """(total_bits, n_bytes_header) per (header, bytes_nn) over the device latents, None where the library refuses the network:
    the rate meter alone, one EncodeBatch, one measure and one wait.  raise_status: a slot the meter leaves with a negative
    status (a latent outside the alphabet) raises it."""
    from .encoder import EncodeBatch

    out = [None] * len(nets)
    with EncodeBatch(device) as enc:
        slots = []
        for i, (header, bytes_nn) in enumerate(nets):
            s, no = refused(enc.add_device, header, bytes_nn, latent_ptrs, owner=owner)
            if not no:
                slots.append((i, s))
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


class NetworkQuantiser:
    """search(): the q-step search of one intra frame's networks on one MI355X."""

    def __init__(self, device: int = 0, max_in_flight_bytes: int = 4 << 30):
        """max_in_flight_bytes: the budget the chunks are sized for with slot_bytes' estimate; not a hard limit."""
        self.device = int(device)
        self.max_in_flight_bytes = int(max_in_flight_bytes)

    @staticmethod
    def slot_bytes(arch: CCHeader, module: int) -> int:
        """Device bytes one candidate of this module is COUNTED with when chunks are sized - an estimate from the architecture,
        not what the handles allocate (their tables, partial sums and the block pool's rounding come on top; measured 17 %
        above the budget on a 1080p frame): a rate-meter slot (ARM, IFCE: the encoder's pair and payload
        buffers) or a given-latents decode slot (latents, dense stack, float output, planes)."""
        n_sym, px = int(arch.n_symbols), int(arch.img_size[0]) * int(arch.img_size[1])
        if module < 2:
            return 16 * n_sym + (64 << 10)
        return n_sym + px * (4 * int(arch.input_feature_synthesis) + 4 * int(arch.out_channels) + 6) + (64 << 10)

    def chunk_size(self, arch: CCHeader, module: int) -> int:
        """Candidates per launch: max_in_flight_bytes over the slot_bytes estimate, at least one."""
        return max(1, self.max_in_flight_bytes // self.slot_bytes(arch, module))

    def search(self, arch: CCHeader, float_values: np.ndarray, latent_ptrs: Sequence[int], source, lmbda: float, sweeps: int = 1,
               fast_path_only: bool = False, owner=None) -> QuantisedNetwork:
        """arch: the architecture (the transmitted fields but the networks' are read); float_values: float32 parameters in
        stream order (writer.network_layout); latent_ptrs: device latents as RdEvaluator.add takes them (int8 [h][w] per grid,
        kept alive by `owner`); source: the FrameData the planes are scored against."""
        import torch

        from .batch import FRAME_DATA_TYPES, DecodeBatch
        from .quality import QualityMeter, _frame_planes
        from .rd import RdEvaluator, rd_cost

        if not np.isfinite(float(lmbda)) or float(lmbda) < 0.0:
            raise ValueError("lmbda must be finite and not negative")
        if source.frame_data_type not in ("rgb", "yuv420", "yuv444"):
            raise ValueError(f"cannot score a {source.frame_data_type} frame")
        if tuple(arch.img_size) != tuple(source.img_size):
            raise ValueError(f"the architecture is {arch.img_size[0]}x{arch.img_size[1]}, the source {source.img_size[0]}x{source.img_size[1]}")
        x = np.ascontiguousarray(float_values, dtype=np.float32).ravel()
        layout = writer.network_layout(arch)
        if x.size != sum(layout):
            raise ValueError("%d parameters, the layout wants %d" % (x.size, sum(layout)))
        ptrs = [int(p) for p in latent_ptrs]
        fdt = FRAME_DATA_TYPES.index(source.frame_data_type)
        dev = torch.device(f"cuda:{self.device}")
        st = torch.cuda.current_stream(self.device).cuda_stream
        src_planes = _frame_planes(source, dev)
        n_samples = [int(t.numel()) for t in src_planes]

        def full(net: _Network):
            with RdEvaluator(self.device) as ev:
                ev.add(net.header, net.bytes_nn, ptrs, source, owner=owner)
                return ev.evaluate(lmbda)[0]

        # what the meter that a module does NOT run would say: the current network's; None until a network has been priced
        state = {"total_bits": None, "sse": None, "n_bytes_header": None}
        start = build_network(arch, x, [writer.q_step_range(g)[0] for g in range(8)], fast_path_only)
        if start is not None and start.feasible:
            c, no = refused(full, start)
            if not no:
                state.update(total_bits=c.rate.total_bits, sse=tuple(c.quality.sse), n_bytes_header=c.rate.n_bytes_header)
        pricing: List[Pricing] = []
        priced: dict = {}   # of the table being chosen from: cell index -> (total_bits, sse, n_bytes_header)

        def rates(nets: List[_Network]):
            return network_rates(self.device, [(net.header, net.bytes_nn) for net in nets], ptrs, owner, st)

        def errors(nets: List[_Network]):
            """sse per plane per network, None where the library refuses it: the float path over the given latents and the
            quality meter alone."""
            out = [None] * len(nets)
            with DecodeBatch(self.device) as dec, QualityMeter(self.device) as meter:
                slots = []
                for i, net in enumerate(nets):
                    s, no = refused(dec.add_latents_device, net.header, net.bytes_nn, ptrs, source.bitdepth, fdt, owner=owner)
                    if not no:
                        slots.append((i, s))
                if slots:
                    dec.run(st)
                    decoded = [[torch.as_tensor(dec.plane_device(s, p), device=dev) for p in range(3)] for _, s in slots]
                    meter.score_planes_async(decoded, [src_planes] * len(slots), [source.bitdepth] * len(slots), False, stream=st)
                    res = meter.finish()
                    dec.wait(st)
                    for (i, _), r in zip(slots, res):
                        out[i] = tuple(int(v) for v in r.sse)
            return out

        def price(m: int, steps: List[int]) -> List[Cell]:
            t0 = time.perf_counter()
            _, gw, gb = MODULES[m]
            pairs = module_cells(m)
            nets = []
            for q_w, q_b in pairs:
                s = list(steps)
                s[gw], s[gb] = q_w, q_b
                nets.append(build_network(arch, x, s, fast_path_only))
            t_built = time.perf_counter()
            need_rate = m < 2 or state["total_bits"] is None
            need_planes = m >= 2 or state["sse"] is None
            chunk = min(self.chunk_size(arch, 0) if need_rate else 1 << 30, self.chunk_size(arch, 2) if need_planes else 1 << 30)
            live = [i for i, n in enumerate(nets) if n is not None and n.feasible]
            priced.clear()
            for at in range(0, len(live), chunk):
                part = live[at:at + chunk]
                r = rates([nets[i] for i in part]) if need_rate else [(state["total_bits"], state["n_bytes_header"])] * len(part)
                e = errors([nets[i] for i in part]) if need_planes else [state["sse"]] * len(part)
                for i, ri, ei in zip(part, r, e):
                    if ri is not None and ei is not None:
                        priced[i] = (ri[0], ei, ri[1])
            cells = []
            for i, (q_w, q_b) in enumerate(pairs):
                if i not in priced:
                    cells.append(Cell(q_w, q_b, False, len(nets[i].bytes_nn) if nets[i] is not None else -1, float("nan"), float("nan"), float("nan")))
                    continue
                total_bits, sse, n_hdr = priced[i]
                mse, bits, cost = rd_cost(sse, n_samples, source.bitdepth, total_bits, len(nets[i].bytes_nn), n_hdr, source.n_pixels, lmbda)
                cells.append(Cell(q_w, q_b, True, len(nets[i].bytes_nn), mse, bits, cost))
            pricing.append(Pricing(time.perf_counter() - t0, t_built - t0, chunk))
            return cells

        def chosen(m: int, k: int) -> None:
            total_bits, sse, n_hdr = priced[k]
            state.update(total_bits=total_bits, sse=sse, n_bytes_header=n_hdr)

        steps, tables = search_steps(price, layout[2] > 0, sweeps, chosen)
        net = build_network(arch, x, steps, fast_path_only)
        if net is None or not net.feasible:
            raise ValueError("no feasible network was found: every candidate of the module that holds the start back is infeasible "
                             "(a payload beyond 16 383 bytes, a refused value or, with fast_path_only, an ARM outside the fast path)")
        return QuantisedNetwork(net.header, net.bytes_nn, net.values, full(net), tables, pricing)
