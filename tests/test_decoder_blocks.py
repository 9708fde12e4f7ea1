"""The decoder wave of the pipelined entropy kernel (ccd_entropy_pipe.hip, decoder_grid): the unrolled symbol blocks that
tools/gen_decoder_block.py writes - table rows asked for two per LDS read, one wait per two symbols - with their exits: the
trampolines' renormalisation, the payload refill (the region is left and entered again inside the batch) and the compiled rare path.

CPU part: the generated text itself (every row register is waited for before it is read), and a replay of the range decoder on the host from the oracle's table indices and latents, which says
at which position of a batch every renormalisation and every payload refill falls - asserted, so that the GPU part (the same
streams, every grid's latents and the consumed word count against the oracle, bit for bit) cannot silently lose that coverage."""
import importlib.util
import os
import re

import numpy as np
import pytest

import producer_cases as pc
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cool_chic_amd", "csrc")

# (h, w): seeds.  272 x 64 and 251 x 33 (w x h) have a streamed body of full 16-symbol batches on grid 0 (w >= 240, h >= 25) and
# 8-symbol parts; its transpose 64 x 272 (longest step 7) and 40 x 12 run 2-pixel tasks; 96 x 40 and 130 x 24 run 4-pixel tasks
# (longest step 10 / 13: the chained 4-symbol parts); 9 x 30 is coded in raster order.  272 x 64 holds 331 payload words - 5
# refills - so 272 x 272 (1871 words, 29 refills) is the stream of the refill test.
SHAPES = {(64, 272): (1,), (272, 64): (1,), (33, 251): (1,), (40, 96): (1,), (24, 130): (2,), (12, 40): (1,), (30, 9): (1,),
          (272, 272): (1,)}
STREAMED = ((64, 272), (33, 251), (272, 272))
REFILLED = ((272, 272),)


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import DecodeBatch, _lib

    _lib.lib()
    return DecodeBatch


# ---- the generated text ----------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("gen_decoder_block", os.path.join(ROOT, "tools", "gen_decoder_block.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _asm(lines):
    return [re.match(r'\s*"(.*)\\n\\t"', l).group(1) for l in lines]


def _regs(operand):
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", operand)
    return {int(m.group(1))} if m else set()


def _check_rows_waited_for(asm, end_label, look=({40, 41, 42, 43},)):
    """Walks a block's straight line up to the label behind its last symbol (LDS answers a wave in order): no instruction may read a
    VGPR that an LDS read still in flight is going to write.  Returns (row reads, waits) seen."""
    in_flight = list(look)  # the look in front of a block asked for rows 0 / 1 last
    n_reads = n_waits = 0
    for ins in asm:
        op, _, rest = ins.partition(" ")
        ops = [o.strip() for o in rest.split(",")] if rest else []
        if op.startswith("ds_read"):
            in_flight.append(_regs(ops[0]))
            n_reads += op != "ds_read_b32"
        elif op.startswith("ds_write"):
            in_flight.append(set())
        elif op == "s_waitcnt":
            k = int(re.search(r"lgkmcnt\((\d+)\)", rest).group(1))
            in_flight = in_flight[len(in_flight) - k:] if k else []
            n_waits += 1
        elif op.startswith("v_"):
            pending = set().union(*in_flight) if in_flight else set()
            for o in ops:
                assert not (_regs(o) & pending), f"{ins}: reads a register an LDS read in flight still writes"
        if ins == "%d:" % end_label:
            break
    return n_reads, n_waits


def test_generated_blocks_wait_for_every_row_they_read():
    """Paired form: 7 row reads and 8 waits in the 16-symbol block (rows 16 / 17 are not asked for), every register waited for
    before its first use - in the full block, both 8-symbol parts and the four 4-symbol parts; the earlier form (one read and
    one wait per symbol), which tools/ubench/dcycle.hip measures against, passes the same walk."""
    g = _generator()
    g.ROWS2 = True
    assert _check_rows_waited_for(_asm(g.block_paired(16, 201)), 316) == (7, 8)
    for label0, lane0 in ((400, 0), (420, 8)):
        reads, waits = _check_rows_waited_for(_asm(g.block_paired(8, 1001, label0=label0, lane0=lane0, part=True, cont=lane0 == 0)), label0 + 8)
        assert (reads, waits) == ((4, 4) if lane0 == 0 else (3, 4))
    for k in range(4):
        reads, waits = _check_rows_waited_for(_asm(g.block_paired(4, 1801, label0=440 + 10 * k, lane0=4 * k, part=True,
                                                                   chain=(450 + 10 * k) if k < 3 else None)), 444 + 10 * k)
        assert (reads, waits) == ((2, 2) if k < 3 else (1, 2))
    g.ROWS2 = False
    assert _check_rows_waited_for(_asm(g.block_paired(16, 201)), 316, ({40, 41}, {42, 43})) == (16, 16)


# ---- streams, the oracle's decode and the replay -----------------------------------------------------------------------------------
_WIDTH = {}


def _decode_order(h, w):
    """(raster index, wavefront step, index within the step, pixels of the step) of the k-th decoded pixel."""
    yy, xx = np.mgrid[0:h, 0:w]
    y, x = yy.ravel(), xx.ravel()
    if w <= 9:
        k = np.arange(h * w)
        return k, k, np.zeros(h * w, np.int64), np.ones(h * w, np.int64)
    c = x + 10 * y
    order = np.lexsort((y, c))
    cs = c[order]
    first = np.searchsorted(cs, cs, side="left")
    count = np.searchsorted(cs, cs, side="right") - first
    return order, cs, np.arange(h * w) - first, count


class _Stream:
    """One stream, what the oracle decodes from it, and the replay of the range decoder (64-bit state, 24-bit precision, 32-bit
    words: new range = (range >> 24) * width; below 2^32 it is shifted up by 32 and the next payload word is taken): per grid,
    in decode order, whether the symbol renormalises and which payload word it takes."""

    def __init__(self, oracle, shape, stream):
        self.shape, self.stream = shape, stream
        self.triple = oracle.split_stream(stream)[1][0][1][0]
        r = oracle.decode_coolchic(*self.triple, stop_after_entropy=True)
        self.latents = [np.array(a) for a in r["latent"]]
        self.words_consumed = r["words_consumed"]
        self.n_words = len(self.triple[2]) // 4
        self.events = []  # (grid, position in its batch / 4-symbol part or -1, that is full, pixels per task, word index taken)
        self.body_events = []  # the same for the streamed body of grid 0: batches cut on the body's pixel index
        rng, word = (1 << 64) - 1, 2
        for g in range(r["n_grids"] - 1, -1, -1):
            h, w = r["grid_hw"][g]
            order, step, k_in_step, n_step = _decode_order(h, w)
            ms = r["mu_scale_idx"][g].astype(np.int64)
            sym = r["latent"][g].ravel()[order].astype(np.int64)
            key = ((ms[:, 0] << 24) | (ms[:, 1] << 8) | (sym + 64)).tolist()
            tp = pc.task_pixels(h, w) if w > 9 else 0
            bpx = 8 if tp == 2 else 16
            body = (230, w + 10 * (h - 24)) if (g == 0 and w > 230 and h >= 25) else (0, 0)
            body_k = 0
            for k, t in enumerate(key):
                if t not in _WIDTH:
                    left, right = oracle.laplace_bounds(t >> 24, (t >> 8) & 0xFFFF, (t & 0xFF) - 64)
                    _WIDTH[t] = right - left
                rng = (rng >> 24) * _WIDTH[t]
                in_body = body[0] <= step[k] < body[1]
                if rng < (1 << 32):
                    rng <<= 32
                    if in_body:
                        self.body_events.append((g, body_k % 16, True, tp, word))
                    elif tp:  # (4-pixel tasks never fill a 16-symbol batch here - steps of 9..24 pixels: position in the PART)
                        cut = 4 if tp == 4 else bpx
                        full = (k_in_step[k] // cut) * cut + cut <= n_step[k]
                        self.events.append((g, int(k_in_step[k] % cut), bool(full), tp, word))
                    else:
                        self.events.append((g, -1, False, tp, word))
                    word += 1
                body_k += in_body
        assert word == self.words_consumed, "the replay and the oracle take the same number of payload words"

    def refills(self):
        """Events that use the last word of a 64-word payload buffer (the first buffer starts at word 2)."""
        return [e for e in self.events + self.body_events if (e[4] - 2) % 64 == 63]


@pytest.fixture(scope="module")
def streams(oracle):
    """Every stream of SHAPES (synth.image_stream: kodim14's networks, its latents tiled and rolled by the seed), decoded once by
    the oracle and replayed once; shared by the tests below."""
    from cool_chic_amd import synth

    return {(shape, seed): _Stream(oracle, shape, synth.image_stream(shape[0], shape[1], seed))
            for shape, seeds in SHAPES.items() for seed in seeds}


@pytest.fixture(scope="module")
def crafted(oracle):
    """272 x 64 with producer_cases.crafted_latents: blocks of symbols outside the decoder's window (the compiled rare path and its
    re-entry in the middle of a batch) between stretches of ordinary symbols."""
    from cool_chic_amd import writer

    bs, _, _ = load_golden("kodim14")
    (fh, ccs), = oracle.split_stream(bs)[1]
    hdr, nn, _ = ccs[0]
    arch = writer.derive_arch(writer.parse_cc_header(hdr), img_size=(64, 272))
    stream = writer.encode_stream(writer.cc_header_bytes(arch), nn, pc.crafted_latents(arch), bitdepth=fh.bitdepth,
                                  frame_data_type=fh.frame_data_type)
    return _Stream(oracle, (64, 272), stream)


def test_renormalisation_falls_on_every_position_of_every_block(streams):
    """A renormalisation at every symbol index 0..15 of the full 16-symbol batches of a streamed body (grid 0 of 272 x 64, 251 x 33
    and 272 x 272: the body is cut into batches on its own pixel index, and only there do 8-pixel tasks fill batches) - whether
    the device takes such a batch whole or as two 8-symbol parts depends on when the producers deliver, and 0..15 covers every
    index of either part; and at every index 0..3 of a full 4-symbol part of the grids on 4-pixel tasks, chained or not.  The
    trampolines therefore re-enter the blocks behind even and behind odd symbols."""
    body, part4 = set(), {}
    for (shape, seed), s in streams.items():
        body |= {e[1] for e in s.body_events}
        part4[shape] = {e[1] for e in s.events if e[2] and e[3] == 4}
        print(shape, seed, "renormalisations", len(s.events) + len(s.body_events), "in the body", len(s.body_events),
              "refills", len(s.refills()), "words", s.n_words)
    assert body == set(range(16)), sorted(body)
    for shape in ((64, 272), (272, 272)):  # (251 x 33: a body of a few steps, 20 renormalisations)
        assert {e[1] for (sh, _), s in streams.items() if sh == shape for e in s.body_events} == set(range(16)), shape
    for shape in ((40, 96), (24, 130)):
        assert part4[shape] == set(range(4)), (shape, sorted(part4[shape]))


def test_refill_falls_on_even_and_odd_and_last_positions(streams):
    """The payload buffer runs out ((word - 2) % 64 == 63 at a renormalisation) behind even and behind odd symbols of a full
    batch, in a batch's last two symbols, and at least 8 times in the 272 x 272 stream; every stream's payload ends inside the
    buffer its last refill loaded (lanes past n_words are set to 0).  A refill leaves the asm region and re-enters it inside
    the batch: rows 0 / 1 of the re-entry come from one paired read, and the 3-copy loop waits for it where it is entered."""
    pos = set()
    for (shape, seed), s in streams.items():
        r = s.refills()
        pos |= {e[1] for e in r if e[2]}
        if shape in REFILLED:
            assert len(r) >= 8, (shape, seed, len(r))
        if r:
            last_base = 2 + 64 * len(r)  # first word of the buffer moved in by the last refill
            assert last_base <= s.n_words + 64 and s.n_words - last_base < 64, (shape, seed, s.n_words, last_base)
    print("refill positions in full batches", sorted(pos))
    assert {p % 2 for p in pos} == {0, 1}
    assert pos & {14, 15}, sorted(pos)


# ---- the device ------------------------------------------------------------------------------------------------------------------
def _check(b, slot, s):
    st = b.slot_stats(slot)
    print(s.shape, "status", b.slot_status(slot), "words", st[1], "streamed grids", st[36], "part batches", st[37], "rare", st[62])
    assert b.slot_status(slot) == 0
    for g, a in enumerate(s.latents):
        assert np.array_equal(b.latent(slot, g), a), f"shape {s.shape} grid {g}"
    assert st[1] == s.words_consumed, (s.shape, st[1], s.words_consumed)
    if s.shape in STREAMED:
        assert st[36] >= 1, f"{s.shape}: no grid was streamed"
        assert st[37] > 0, f"{s.shape}: no batch was decoded part by part"
    return st


def _run(gpu, items):
    b = gpu(0)
    for s in items:
        b.add(*s.triple, 8, 0)
    b.run()
    b.wait()
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("key", [(shape, seed) for shape, seeds in SHAPES.items() for seed in seeds])
def test_stream_alone(gpu, streams, key):
    """One stream in its own batch: every grid's latents and the consumed word count against the oracle."""
    b = _run(gpu, [streams[key]])
    try:
        _check(b, 0, streams[key])
    finally:
        b.close()


@pytest.mark.gpu
def test_streams_together_and_twice(gpu, streams):
    """One stream of each shape in one batch (8 slots), run twice: the same checks per slot, and the second run's latents are the
    first's."""
    items = [streams[k] for k in streams]
    assert len(items) == 8
    b = _run(gpu, items)
    try:
        first = []
        for i, s in enumerate(items):
            _check(b, i, s)
            first.append([np.array(b.latent(i, g)) for g in range(len(s.latents))])
        b.run()
        b.wait()
        for i, s in enumerate(items):
            _check(b, i, s)
            for g, a in enumerate(first[i]):
                assert np.array_equal(b.latent(i, g), a), f"run 2 differs: shape {s.shape} grid {g}"
    finally:
        b.close()


@pytest.mark.gpu
def test_rare_path_re_entry_inside_a_batch(gpu, crafted):
    """Symbols outside the window leave the region for the compiled path and come back inside their batch (slot_stats[62])."""
    b = _run(gpu, [crafted])
    try:
        st = _check(b, 0, crafted)
        assert st[62] > 0
    finally:
        b.close()
