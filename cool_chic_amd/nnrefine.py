"""ArmRefiner, RateRefiner: a +-1 descent over the transmitted integers of a cool-chic's rate networks - the ARM,
the IFCE (4.21) or both - after the steps are chosen.

These integers change only the rate: the planes, the squared error and the header size stay what they were (the IFCE's change
the features the ARM reads and nothing else), so "better" is fewer bits, total_bits + 8 * len(bytes_nn) in rd.rd_cost's terms,
for every lambda > 0, and neither a source picture nor a reconstruction is needed - the same code serves an intra frame and both
cool-chics of a P / B frame.  Every step asks the device for the exact change of the latents' model bits for -1 and +1 at every
integer (EncodeBatch.measure_param_deltas, measure_ifce_deltas), adds the exact change of the payload's size, picks moves, and
accepts them only if the existing meter says that the objective fell.

`expgol_bit_deltas`, `payload_byte_deltas`, their `rate_` forms over groups 0 .. 3 and `pick_moves` are pure functions, testable
without a device."""
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

from . import writer
from ._lib import CCHeader
from .nnquant import network_rates

MAX_ORDER = 12  # Exp-Golomb orders the header can name (ccd_network_best_expgol)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


class Move(NamedTuple):
    index: int      # ARM integer, stream order
    sign: int       # -1 / +1
    delta: float    # the change of the objective the tables promise for this move alone


class StepLog(NamedTuple):
    """One accepted step.  `rejected`: the larger batches tried first, [(number of moves, predicted, true objective)]."""
    moves: List[Move]
    predicted: float        # objective before + the latent deltas of the moves + 8 x the exact change of the payload's bytes
    objective: float        # what the meter found: total_bits + 8 * len(bytes_nn)
    total_bits: float
    n_bytes_nn: int
    moved: int              # symbols whose interval the moves change, summed over the moves (the table's `moved`)
    rejected: List[Tuple[int, float, float]]


class RefinedNetwork(NamedTuple):
    header: CCHeader        # arch with nn_expgol_cnt, nn_n_bytes and nn_n_bit_pad set
    bytes_nn: bytes
    values: np.ndarray      # int32, stream order
    start_objective: float  # of the network given, with its best Exp-Golomb orders
    log: List[StepLog]      # the accepted steps; the last one's objective is the result's
    stopped: str            # "max_steps", "no move promises a gain" or "the best single move does not lower the objective"


def _code_len(v: np.ndarray, count) -> np.ndarray:
    """Bits of the Exp-Golomb code of order `count` for the integers v (ccd_encode_network): the sign folded into the LSB,
    u + 2^count in binary behind floor(log2(u + 2^count)) - count zeros."""
    v = np.asarray(v, np.int64)
    u = np.where(v <= 0, -2 * v, 2 * v - 1)
    y = u + (np.int64(1) << np.asarray(count, np.int64))
    length = np.frexp(y.astype(np.float64))[1].astype(np.int64) - 1  # floor(log2 y): exact, y < 2^34
    return 2 * length - count + 1


def _arm_groups(arch: CCHeader, values: np.ndarray):
    layout = writer.network_layout(arch)
    v = np.asarray(values)
    if v.ndim != 1 or v.size != sum(layout):
        raise ValueError("%d values, the layout wants %d" % (v.size, sum(layout)))
    return layout, v.astype(np.int64)


def _expgol_bit_deltas(arch: CCHeader, values: np.ndarray, n_groups: int) -> np.ndarray:
    layout, v = _arm_groups(arch, values)
    n_arm = sum(layout[:n_groups])  # the groups are contiguous in stream order
    count = np.repeat(np.array([arch.nn_expgol_cnt[g] for g in range(n_groups)], np.int64), layout[:n_groups])
    a = v[:n_arm]
    base = _code_len(a, count)
    out = np.empty((n_arm, 2), np.float64)
    for j, s in enumerate((-1, 1)):
        out[:, j] = _code_len(a + s, count) - base
        out[(a + s < INT32_MIN) | (a + s > INT32_MAX), j] = np.inf
    return out


def expgol_bit_deltas(arch: CCHeader, values: np.ndarray) -> np.ndarray:
    """float64 [n_arm][2] (-1 first): the exact change of the NN payload's bit count before padding if ARM integer k alone were
    values[k] - 1 / + 1, under the orders in arch.nn_expgol_cnt.  +inf where the integer would leave int32."""
    return _expgol_bit_deltas(arch, values, 2)


def rate_expgol_bit_deltas(arch: CCHeader, values: np.ndarray) -> np.ndarray:
    """expgol_bit_deltas for both rate networks: float64 [n_arm + n_ifce][2], groups 0 .. 3 of writer.network_layout (the ARM's
    weights and biases, then the IFCE's), which follow each other in the stream: row k is values[k]."""
    return _expgol_bit_deltas(arch, values, 4)


def _payload_byte_deltas(arch: CCHeader, values: np.ndarray, n_groups: int) -> np.ndarray:
    layout, v = _arm_groups(arch, values)
    n_arm = sum(layout[:n_groups])
    orders = np.arange(MAX_ORDER + 1, dtype=np.int64)
    at = np.cumsum([0] + layout)
    best = [int(_code_len(v[at[g]:at[g + 1], None], orders[None, :]).sum(axis=0).min()) if layout[g] else 0 for g in range(8)]
    total = sum(best)
    out = np.empty((n_arm, 2), np.float64)
    for g in range(n_groups):
        lo, hi = int(at[g]), int(at[g + 1])
        a = v[lo:hi]
        per_order = _code_len(a[:, None], orders[None, :])            # [n][13]
        group = per_order.sum(axis=0)                                  # [13]
        for j, s in enumerate((-1, 1)):
            moved = group[None, :] - per_order + _code_len((a + s)[:, None], orders[None, :])
            bits = total - best[g] + moved.min(axis=1)
            out[lo:hi, j] = 8.0 * (-(-bits // 8) - -(-total // 8))
            out[lo:hi, j][(a + s < INT32_MIN) | (a + s > INT32_MAX)] = np.inf
    return out


def payload_byte_deltas(arch: CCHeader, values: np.ndarray) -> np.ndarray:
    """float64 [n_arm][2]: the exact change of 8 * len(bytes_nn) for the same single moves when every group's order is chosen
    again (writer.best_expgol, then writer.encode_network: what ArmRefiner builds), relative to `values` with ITS best orders.
    A group's bits at every order change by the one code that moved, so the new minimum needs no second pass over the group."""
    return _payload_byte_deltas(arch, values, 2)


def rate_payload_byte_deltas(arch: CCHeader, values: np.ndarray) -> np.ndarray:
    """payload_byte_deltas for both rate networks: float64 [n_arm + n_ifce][2], groups 0 .. 3."""
    return _payload_byte_deltas(arch, values, 4)


def pick_moves(d_latent: np.ndarray, d_nn: np.ndarray, max_moves: int) -> List[Move]:
    """At most `max_moves` moves from two [n][2] tables (-1 first) whose sum is what a move alone changes the objective by: at
    most one per parameter, only moves with a negative sum, best first; ties go to the lower index, then to -1."""
    total = np.asarray(d_latent, np.float64) + np.asarray(d_nn, np.float64)
    if total.ndim != 2 or total.shape[1] != 2:
        raise ValueError("tables of [n][2] entries")
    moves = []
    for k in range(total.shape[0]):
        m, p = float(total[k, 0]), float(total[k, 1])
        best = None
        if m < 0.0:
            best = (m, k, -1)
        if p < 0.0 and (best is None or p < m):
            best = (p, k, 1)
        if best is not None:
            moves.append(best)
    moves.sort()
    return [Move(k, s, d) for d, k, s in moves[:max(int(max_moves), 0)]]


def build_candidate(arch: CCHeader, values: np.ndarray):
    """(header, bytes_nn) of `values` with their best Exp-Golomb orders: a copy of arch with nn_expgol_cnt, nn_n_bytes and
    nn_n_bit_pad set."""
    h = CCHeader.from_buffer_copy(bytes(arch))
    orders, _ = writer.best_expgol(h, values)
    for g in range(8):
        h.nn_expgol_cnt[g] = orders[g]
    return h, writer.encode_network(h, values)


class ArmRefiner:
    """refine(): the +-1 descent over the transmitted integers of the rate networks in `modules` - "arm", "ifce" or both - of one
    cool-chic on one MI355X.  ArmRefiner(device) refines the ARM alone; RateRefiner is this class with both
    modules as the default (4.21).  Groups 0 .. 3 are contiguous in the stream, so a Move.index is an index into `values` for
    both modules; every step takes the tables of the modules refined, makes ONE pick_moves over their rows and builds the
    candidate with all orders chosen again."""

    def __init__(self, device: int = 0, modules: Sequence[str] = ("arm",)):
        self.device = int(device)
        self.modules = tuple(modules)
        if not self.modules or any(m not in ("arm", "ifce") for m in self.modules) or len(set(self.modules)) != len(self.modules):
            raise ValueError('modules: "arm", "ifce" or both')

    def _n_params(self, h: CCHeader) -> int:
        """Rows the table of _table() has, the ARM's and then the IFCE's: the integers refine() may move are values[:this]."""
        return sum(writer.network_layout(h)[:4])

    def _nn_deltas(self, h: CCHeader, values: np.ndarray) -> np.ndarray:
        """The exact change of 8 * len(bytes_nn) for every row and sign of the table (rate_payload_byte_deltas), +inf in the
        rows of a module that is not refined: whatever the table holds there, pick_moves never takes such a row."""
        out = rate_payload_byte_deltas(h, values)
        n_arm = sum(writer.network_layout(h)[:2])
        if "arm" not in self.modules:
            out[:n_arm] = np.inf
        if "ifce" not in self.modules:
            out[n_arm:] = np.inf
        return out

    def _table(self, h: CCHeader, nn: bytes, ptrs, owner, stream):
        """(total_bits, ParamDeltas over [n_arm + n_ifce] rows) of the network as it stands: one measure per module refined
        (EncodeBatch.measure_param_deltas, measure_ifce_deltas) on one handle; the rows of the other module hold +inf, 0, 0.
        refine() calls it through self, so a test can put a made-up table in its place."""
        from .encoder import EncodeBatch, ParamDeltas

        n_arm, n = sum(writer.network_layout(h)[:2]), self._n_params(h)
        bits = np.full((n, 2), np.inf, np.float64)
        sum_width, moved = np.zeros((n, 2), np.int64), np.zeros((n, 2), np.int64)
        with EncodeBatch(self.device) as enc:
            slot = enc.add_device(h, nn, ptrs, owner=owner)
            for module in self.modules:
                if module == "arm":
                    enc.measure_param_deltas(stream)
                    enc.wait(stream)
                    t, rows = enc.param_deltas(slot), slice(0, n_arm)
                else:
                    enc.measure_ifce_deltas(stream)
                    enc.wait(stream)
                    t, rows = enc.ifce_deltas(slot), slice(n_arm, n)
                if t.first != 0 or t.bits.shape[0] != rows.stop - rows.start:
                    raise ValueError("the %s table does not cover the module" % module)
                bits[rows], sum_width[rows], moved[rows] = t.bits, t.sum_width, t.moved
            return enc.rate(slot).total_bits, ParamDeltas(0, bits, sum_width, moved)

    def _price(self, h: CCHeader, nn: bytes, ptrs, owner, stream):
        """total_bits of a candidate by the existing meter; None where the library refuses the network."""
        r, = network_rates(self.device, [(h, nn)], ptrs, owner, stream, raise_status=True)
        return None if r is None else r[0]

    def refine(self, arch: CCHeader, values: np.ndarray, latent_ptrs: Sequence[int], max_steps: int, batch: int = 1, owner=None,
               stream: int = 0) -> RefinedNetwork:
        """arch: the architecture with its quantisation steps (the orders and the payload size are set here); values: int32 in
        stream order; latent_ptrs: device latents as EncodeBatch.add_device takes them (kept alive by `owner`).  Every step
        builds the table, picks up to `batch` moves, prices the candidate (orders chosen again, which never adds bytes) with the
        meter and accepts it only if the objective falls; otherwise the batch is halved down to the single best move, and when
        that does not lower the objective either the descent stops.  The objective never rises."""
        if int(batch) < 1 or int(max_steps) < 0:
            raise ValueError("batch >= 1 and max_steps >= 0")
        ptrs = [int(p) for p in latent_ptrs]
        values = np.ascontiguousarray(values, dtype=np.int32).copy()
        h, nn = build_candidate(arch, values)
        if len(nn) > writer.MAX_NN_BYTES:
            raise ValueError("the network's payload is beyond the header's 16 383 bytes")
        log: List[StepLog] = []
        start = None
        stopped = "max_steps"
        for _ in range(int(max_steps)):
            base_bits, table = self._table(h, nn, ptrs, owner, stream)
            objective = base_bits + 8.0 * len(nn)
            if start is None:
                start = objective
            if table.first != 0 or table.bits.shape[0] != self._n_params(h):
                raise ValueError("the table does not cover the ARM and the IFCE")
            moves = pick_moves(table.bits, self._nn_deltas(h, values), int(batch))
            if not moves:
                stopped = "no move promises a gain"
                break
            rejected = []
            n = len(moves)
            accepted = None
            while True:
                cand = values.copy()
                for m in moves[:n]:
                    cand[m.index] += m.sign
                ch, cnn = build_candidate(arch, cand)
                predicted = base_bits + float(sum(table.bits[m.index, (m.sign + 1) // 2] for m in moves[:n])) + 8.0 * len(cnn)
                bits = self._price(ch, cnn, ptrs, owner, stream) if len(cnn) <= writer.MAX_NN_BYTES else None
                true = float("inf") if bits is None else bits + 8.0 * len(cnn)
                if true < objective:
                    moved = int(sum(int(table.moved[m.index, (m.sign + 1) // 2]) for m in moves[:n]))
                    accepted = StepLog(list(moves[:n]), predicted, true, bits, len(cnn), moved, rejected)
                    h, nn, values = ch, cnn, cand
                    break
                rejected.append((n, predicted, true))
                if n == 1:
                    break
                n //= 2
            if accepted is None:
                stopped = "the best single move does not lower the objective"
                break
            log.append(accepted)
        if start is None:  # max_steps == 0
            bits = self._price(h, nn, ptrs, owner, stream)
            start = float("inf") if bits is None else bits + 8.0 * len(nn)
        return RefinedNetwork(h, nn, values, start, log, stopped)


class RateRefiner(ArmRefiner):
    """ArmRefiner over BOTH rate networks unless told otherwise: modules=("ifce",) refines the IFCE alone, ("arm",) is
    ArmRefiner.  The IFCE's integers change the features the ARM reads and nothing else, so the objective, the acceptance rule
    and the meter are the same."""

    def __init__(self, device: int = 0, modules: Sequence[str] = ("arm", "ifce")):
        super().__init__(device, modules)
