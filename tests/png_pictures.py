"""Pictures and readers shared by tests/test_png.py and tests/test_png_lz77.py."""
import io

import numpy as np

SIZES = [(1, 1), (1, 7), (7, 1), (2, 3), (17, 33), (64, 64), (100, 300), (33, 1111)]


def _pictures(h, w, seed=0):
    rng = np.random.default_rng(seed + 7919 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(yy * 3 + xx) % 256, (yy + xx * 2) % 256, (yy * xx) % 256]).astype(np.uint8)
    photo = np.clip(smooth.astype(np.int32) // 2 + rng.normal(0, 6, (3, h, w)).round().astype(np.int32) + 40, 0, 255).astype(np.uint8)
    return {
        "random": rng.integers(0, 256, (3, h, w), dtype=np.uint8),
        "smooth": smooth,
        "photo": photo,
        "zeros": np.zeros((3, h, w), np.uint8),
        # counts falling off geometrically: optimal codes up to 15 bits deep
        "skewed": np.minimum(rng.geometric(0.55, (3, h, w)) * 3, 255).astype(np.uint8),
    }


def _read_png(png: bytes) -> np.ndarray:
    from PIL import Image

    im = Image.open(io.BytesIO(png))
    assert im.mode == "RGB"
    return np.asarray(im).transpose(2, 0, 1)


def _fibonacci_row(nval=17, seed=0):
    """One row, one deflate block of 6.7 KB, whose optimal Huffman code is deeper than 15 bits (the test asserts that from
    the CPU restatement before it uses it).  Byte values 0, 1, -1, 2, -2, ... occur 1, 2, 3, 5, 8, ... times, the rarest
    first: with the end-of-block symbol's 1 in front every count exceeds the sum of all counts two or more places
    before it, so every merge of the Huffman construction takes the tree built so far and one leaf.  The values are
    shuffled: the bytes are centred on 0 and independent, which makes filter None the cheapest and keeps the counts."""
    fib = [1, 2]
    while len(fib) < nval:
        fib.append(fib[-1] + fib[-2])
    signed = [(r + 1) // 2 * (1 if r % 2 else -1) for r in range(nval)]  # 0, 1, -1, 2, -2, ...
    vals = np.repeat(np.array(signed[::-1], np.int64) % 256, fib).astype(np.uint8)
    np.random.default_rng(seed).shuffle(vals)
    vals = np.concatenate([vals, np.zeros(-vals.size % 3, np.uint8)])
    return np.ascontiguousarray(vals.reshape(1, -1, 3).transpose(2, 0, 1))


def _unlimited_depths(code_lengths, hist):
    """Depths of the Huffman tree `code_lengths` builds before it limits them: the same function with the limit (which
    both restatements read from oracle.png_pack.MAX_BITS at every call) out of reach."""
    from oracle import png_pack

    limit = png_pack.MAX_BITS
    png_pack.MAX_BITS = 64
    try:
        return code_lengths(hist)
    finally:
        png_pack.MAX_BITS = limit


def _deep_litlen_row(seed=0):
    """One row (one deflate block of 32 KB) that takes the LZ77 coding with a literal/length tree 16 deep before the limit
    (the test asserts both from the CPU restatement before it uses the picture).  The scanline is designed, then the
    Sub filter is inverted: runs of equal bytes over 128 byte values.  The first run of a value (11 bytes) is one
    literal and one match of length 10 at distance 1; every later run of 3..10 bytes is one match of exactly its
    length, because (a) the nearest earlier positions with its trigram hold one with at least as many bytes left, and
    (b) no two runs' ends join the same pair of values, so that no match crosses a run's end.
    So the tree has 130 symbols of count 1 at the bottom (the literals, the filter byte, end-of-block: 8 levels) and
    above them the length symbols of 10, 9, ..., 3, whose counts each exceed the weight of the tree two merges
    earlier (8 more levels)."""
    rng = np.random.default_rng(seed)
    values = [v % 256 for v in list(range(-64, 0)) + list(range(2, 66))]  # neither 0 nor the filter byte 1
    runs_of = {10: 132 - len(values), 9: 132, 8: 264, 7: 396, 6: 660, 5: 1056, 4: 1716, 3: 2772}
    total = 11 * len(values) + sum(r * c for r, c in runs_of.items())
    runs_of[4] += -total % 3  # whole pixels; the chain above tolerates it
    body = np.repeat(list(runs_of), list(runs_of.values()))  # longest first: a run's source is never shorter than it
    tail = {b: [] for b in values}  # per value: (bytes left in the run, run) at its 8 latest trigram positions
    pairs = set()                   # (value, value behind it) of every run's end: none occurs twice
    out, run, prev = [], 0, None
    for r, fixed in [(11, b) for b in values] + [(int(r), None) for r in body]:
        if fixed is None:
            fit = [b for b in values if b != prev and (prev, b) not in pairs and max(q for q, _ in tail[b][-8:]) >= r]
            b = fit[rng.integers(len(fit))]
        else:
            b = fixed
        pairs.add((prev, b))
        tail[b] = (tail[b] + [(q, run) for q in range(r, 2, -1)])[-8:]
        out += [b] * r
        prev, run = b, run + 1
    d = np.array(out, np.int64).reshape(-1, 3)
    return np.ascontiguousarray((np.cumsum(d, axis=0) % 256).astype(np.uint8).T.reshape(3, 1, -1))
