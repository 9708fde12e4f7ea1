"""CPU restatement of the level-1 (LZ77) PNG packer (cool_chic_amd/csrc/ccd_png.hip, level 1), numpy + small Python loops.

TEST INFRASTRUCTURE: only tests import this module; the product package never does.

Level 1 keeps everything of level 0 (oracle/png_pack.py): filters, rows per deflate block, IHDR/IDAT/IEND, zlib header,
Adler-32, CRC-32.  Only the body of each deflate block changes, and only where it gets smaller.  The canon:
  match    inside one deflate block only.  Position i has a key if i + 2 < n; its bucket is
           h = ((b0 << 16 | b1 << 8 | b2) * 0x9E3779B1 mod 2^32) >> 20 (12 bits).  Candidates are the K = 8 nearest
           earlier positions j of the same bucket, kept while i - j <= 32768; a candidate counts if its 3 bytes equal
           those at i.  Length = common prefix, capped at 258 and at the end of the block (overlap allowed).  Best =
           longest, ties to the nearest.  Shorter than 3 is no match; length 3 at a distance > 4096 is dropped.
  parse    lazy-1: at i with a match of length L, a literal if the match at i + 1 is longer than L, else the match
           (advance by L); no match -> literal.  next(i) depends on i alone.
  code     dynamic Huffman, HLIT = 286, HDIST = 30, the code-length code of level 0 (4-bit codes for the lengths
           0..15); both trees by the Moffat-Katajainen construction limited to 15 bits, canonical codes.  A single
           used distance symbol gets length 1.
  choice   a block whose exact LZ77 bit count is >= its level-0 bit count is written exactly as level 0 writes it.
"""
import struct

import numpy as np

from oracle import png_pack as P

K_CAND = 8
HASH_MUL = 0x9E3779B1
HASH_SHIFT = 20
WINDOW = 32768
MAX_MATCH = 258
FAR_3 = 4096                                       # length-3 matches farther than this are dropped
NLL, NDIST = 286, 30
HEADER_BITS_LZ = 3 + 5 + 5 + 4 + 19 * 3 + (NLL + NDIST) * 4  # 1338 bits in front of the first token

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]


# ------------------------------------------------------------------------------------------------ matcher
def buckets(data: np.ndarray) -> np.ndarray:
    """12-bit bucket of every position that has a key (i + 2 < n)."""
    d = data.astype(np.uint64)
    key = (d[:-2] << 16) | (d[1:-1] << 8) | d[2:]
    return (((key * HASH_MUL) & 0xFFFFFFFF) >> HASH_SHIFT).astype(np.int64)


def matches(data: np.ndarray, k_cand: int = K_CAND):
    """data: one block's filtered scanlines (uint8) -> (length, distance) per position, 0 where there is no match."""
    n = data.size
    mlen = np.zeros(n, np.int64)
    mdist = np.zeros(n, np.int64)
    if n < 4:
        return mlen, mdist
    h = buckets(data)
    nk = h.size
    order = np.argsort(h, kind="stable")           # positions grouped by bucket, ascending inside a bucket
    hs = h[order]
    d32 = data.astype(np.int64)
    key3 = (d32[:-2] << 16) | (d32[1:-1] << 8) | d32[2:]
    best_l = np.zeros(nk, np.int64)
    best_d = np.zeros(nk, np.int64)
    lim = np.minimum(MAX_MATCH, n - np.arange(nk))
    for k in range(1, k_cand + 1):                  # k-th nearest earlier position of the same bucket
        cand = np.full(nk, -1, np.int64)
        same = np.zeros(nk, bool)
        same[k:] = hs[k:] == hs[:-k]
        cand[order[k:][same[k:]]] = order[:-k][same[k:]]
        i = np.nonzero(cand >= 0)[0]
        j = cand[i]
        ok = (i - j <= WINDOW) & (key3[j] == key3[i])
        i, j = i[ok], j[ok]
        ln = np.full(i.size, 3, np.int64)
        act = np.nonzero(ln < lim[i])[0]
        while act.size:                              # common prefix, <= 255 more steps
            ia, ja, la = i[act], j[act], ln[act]
            eq = d32[ja + la] == d32[ia + la]
            ln[act[eq]] += 1
            act = act[eq]
            act = act[ln[act] < lim[i[act]]]
        better = ln > best_l[i]                      # strictly longer: ties stay with the nearer candidate
        best_l[i[better]] = ln[better]
        best_d[i[better]] = (i - j)[better]
    drop = (best_l < 3) | ((best_l == 3) & (best_d > FAR_3))
    best_l[drop] = 0
    best_d[drop] = 0
    mlen[:nk] = best_l
    mdist[:nk] = best_d
    return mlen, mdist


def parse(mlen: np.ndarray, mdist: np.ndarray):
    """Lazy-1 parse -> (token start positions, length per token (0 = literal), distance per token)."""
    n = mlen.size
    nxt_l = np.append(mlen[1:], 0)
    take = (mlen >= 3) & (nxt_l <= mlen)
    step = np.where(take, mlen, 1)
    pos = []
    i = 0
    while i < n:
        pos.append(i)
        i += int(step[i])
    pos = np.asarray(pos, np.int64)
    L = np.where(take[pos], mlen[pos], 0)
    D = np.where(take[pos], mdist[pos], 0)
    return pos, L, D


def len_sym(L):
    idx = np.searchsorted(LBASE, L, side="right") - 1
    return 257 + idx, np.asarray(LEXT)[idx], L - np.asarray(LBASE)[idx]


def dist_sym(D):
    idx = np.searchsorted(DBASE, D, side="right") - 1
    return idx, np.asarray(DEXT)[idx], D - np.asarray(DBASE)[idx]


# ------------------------------------------------------------------------------------------------ Huffman
def code_lengths(hist) -> np.ndarray:
    """oracle/png_pack.code_lengths for any alphabet size: optimal lengths (Moffat-Katajainen on the used symbols
    sorted by (count, symbol)), limited to 15 bits, rarest symbols longest.  One used symbol gets length 1; none,
    all zero."""
    hist = np.asarray(hist, np.int64)
    lens = np.zeros(hist.size, np.int32)
    used = sorted((int(c), s) for s, c in enumerate(hist) if c > 0)
    m = len(used)
    if m < 2:
        if m:
            lens[used[0][1]] = 1
        return lens
    A = [cnt for cnt, _ in used]
    A[0] += A[1]
    root, leaf = 0, 2
    for nxt in range(1, m - 1):
        if leaf >= m or A[root] < A[leaf]:
            A[nxt] = A[root]
            A[root] = nxt
            root += 1
        else:
            A[nxt] = A[leaf]
            leaf += 1
        if leaf >= m or (root < nxt and A[root] < A[leaf]):
            A[nxt] += A[root]
            A[root] = nxt
            root += 1
        else:
            A[nxt] += A[leaf]
            leaf += 1
    A[m - 2] = 0
    for nxt in range(m - 3, -1, -1):
        A[nxt] = A[A[nxt]] + 1
    avbl, usedn, dpth, root, nxt = 1, 0, 0, m - 2, m - 1
    while avbl > 0:
        while root >= 0 and A[root] == dpth:
            usedn += 1
            root -= 1
        while avbl > usedn:
            A[nxt] = dpth
            nxt -= 1
            avbl -= 1
        avbl = 2 * usedn
        dpth += 1
        usedn = 0
    num = [0] * (P.MAX_BITS + 1)
    for ln in A:
        num[min(ln, P.MAX_BITS)] += 1
    total = sum(num[ln] << (P.MAX_BITS - ln) for ln in range(1, P.MAX_BITS + 1))
    while total != 1 << P.MAX_BITS:
        num[P.MAX_BITS] -= 1
        for ln in range(P.MAX_BITS - 1, 0, -1):
            if num[ln]:
                num[ln] -= 1
                num[ln + 1] += 2
                break
        total -= 1
    j = 0
    for ln in range(P.MAX_BITS, 0, -1):
        for _ in range(num[ln]):
            lens[used[j][1]] = ln
            j += 1
    assert j == m
    return lens


def canonical_codes(lens: np.ndarray) -> np.ndarray:
    bl_count = np.bincount(lens, minlength=P.MAX_BITS + 1)
    next_code = [0] * (P.MAX_BITS + 2)
    code = 0
    for bits in range(1, P.MAX_BITS + 1):
        code = (code + (bl_count[bits - 1] if bits > 1 else 0)) << 1
        next_code[bits] = code
    codes = np.zeros(lens.size, np.int64)
    for s in range(lens.size):
        ln = int(lens[s])
        if ln:
            codes[s] = P._rev(next_code[ln], ln)
            next_code[ln] += 1
    return codes


# ------------------------------------------------------------------------------------------------ blocks
def lz77_block(data: np.ndarray, k_cand: int = K_CAND):
    """One block -> (exact bit count, list of (values, nbits) arrays to emit after BFINAL) for the LZ77 coding."""
    mlen, mdist = matches(data, k_cand)
    pos, L, D = parse(mlen, mdist)
    lit = L == 0
    sym = np.where(lit, data[pos].astype(np.int64), 0)
    ls, le, lv = len_sym(np.where(lit, 3, L))
    ds, de, dv = dist_sym(np.where(lit, 1, D))
    sym = np.where(lit, sym, ls)
    hll = np.bincount(sym, minlength=NLL)
    hll[256] += 1
    hd = np.bincount(ds[~lit], minlength=NDIST)
    lens_ll, lens_d = code_lengths(hll), code_lengths(hd)
    c_ll, c_d = canonical_codes(lens_ll), canonical_codes(lens_d)
    extra = int(le[~lit].sum() + de[~lit].sum())
    bits = HEADER_BITS_LZ + int((hll * lens_ll).sum()) + int((hd * lens_d).sum()) + extra
    # token stream: per token up to 4 pieces (code, length extra, distance code, distance extra)
    t = pos.size
    vals = np.zeros((t, 4), np.int64)
    nb = np.zeros((t, 4), np.int64)
    vals[:, 0], nb[:, 0] = c_ll[sym], lens_ll[sym]
    m = ~lit
    vals[m, 1], nb[m, 1] = lv[m], le[m]
    vals[m, 2], nb[m, 2] = c_d[ds[m]], lens_d[ds[m]]
    vals[m, 3], nb[m, 3] = dv[m], de[m]
    return bits, (lens_ll, lens_d, vals.reshape(-1), nb.reshape(-1), int(c_ll[256]), int(lens_ll[256])), (pos, L, D)


def deflate(scan: np.ndarray, w: int, k_cand: int = K_CAND):
    """Filtered scanlines [H, 1+3W] -> (deflate bytes, per-block (bits, 'lz' | 'lit'))."""
    h = scan.shape[0]
    R = P.rows_per_block(w)
    nblk = (h + R - 1) // R
    out = P._Bits(scan.size * 15 + nblk * (HEADER_BITS_LZ + 15) + 64)
    info = []
    for k in range(nblk):
        data = scan[k * R:(k + 1) * R].reshape(-1)
        hist = np.bincount(data, minlength=257)
        hist[256] = 1
        lens = P.code_lengths(hist)
        lit_bits = P.HEADER_BITS + int((hist * lens).sum())
        lz_bits, lz, _ = lz77_block(data, k_cand)
        p0 = out.pos
        out.put(1 if k == nblk - 1 else 0, 1)
        out.put(2, 2)
        if lz_bits < lit_bits:
            lens_ll, lens_d, vals, nb, eob_code, eob_len = lz
            out.put(NLL - 257, 5)
            out.put(NDIST - 1, 5)
            out.put(15, 4)
            for s in P.CL_ORDER:
                out.put(0 if s >= 16 else 4, 3)
            for v in list(lens_ll) + list(lens_d):
                out.put(P._rev(int(v), 4), 4)
            sel = nb > 0
            out.put_many(vals[sel], nb[sel])
            out.put(eob_code, eob_len)
            info.append((lz_bits, "lz"))
            assert out.pos - p0 == lz_bits
        else:
            codes = P.canonical_codes(lens)
            out.put(0, 5)
            out.put(0, 5)
            out.put(15, 4)
            for s in P.CL_ORDER:
                out.put(0 if s >= 16 else 4, 3)
            for s in range(258):
                out.put(P._rev(int(lens[s]) if s < 257 else 0, 4), 4)
            out.put_many(codes[data], lens[data])
            out.put(int(codes[256]), int(lens[256]))
            info.append((lit_bits, "lit"))
            assert out.pos - p0 == lit_bits
    n_bytes = (out.pos + 7) // 8
    return np.packbits(out.bits[: n_bytes * 8], bitorder="little").tobytes(), info


def pack_rgb8(planes, k_cand: int = K_CAND, info: list = None) -> bytes:
    """planes: [3, H, W] uint8 (r, g, b) -> level-1 PNG bytes.  `info`, if given, receives the per-block choices."""
    planes = np.asarray(planes)
    assert planes.dtype == np.uint8 and planes.ndim == 3 and planes.shape[0] == 3
    _, h, w = planes.shape
    img = np.ascontiguousarray(planes.transpose(1, 2, 0))
    scan, _ = P.filter_rows(img)
    body, blocks = deflate(scan, w, k_cand)
    if info is not None:
        info.extend(blocks)
    z = b"\x78\x01" + body + struct.pack(">I", P.adler32_rows(scan))
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    png = b"\x89PNG\r\n\x1a\n" + P._chunk(b"IHDR", ihdr) + P._chunk(b"IDAT", z) + P._chunk(b"IEND", b"")
    assert len(png) <= P.bound(h, w)
    return png
