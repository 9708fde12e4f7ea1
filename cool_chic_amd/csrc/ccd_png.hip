// ccd_png.hip - PNG packing of decoded 8-bit RGB planes on the device.
//
// Reference behaviour: coolchic/io/format/png.py:44-62 (write_png: [1,3,H,W] float in [0,1] -> HWC uint8 -> PIL save,
// i.e. zlib deflate on the host).  The integer planes already exist on the device (ccd_batch_plane); this file turns
// them into the bytes of a .png there, so that only the compressed file crosses PCIe and no host core runs zlib.
// PNG bytes are not normative (any conforming zlib stream of the filtered scanlines is the same picture): the device
// does not imitate zlib's LZ77 choices.  Parity bar (tests/test_gpu_parity.py): the picture PIL reads back is
// pixel-exact, and the bytes equal those of the CPU restatement oracle/png_pack.py (all steps are integer).
//
// Format: signature, IHDR, one IDAT with a zlib stream (0x78 0x01) of the filtered scanlines, IEND.
//   filter   per row the one of None/Sub/Up/Average/Paeth with the smallest sum of absolute signed residuals
//   deflate  rows grouped into blocks of rows_per_block(w) rows (about 32 KB of scanlines); every block is a
//            dynamic-Huffman block of literals only + end-of-block: HLIT = 257, HDIST = 1 (length 0), code-length
//            alphabet = 4-bit codes for the lengths 0..15, no run-length symbols; literal lengths are optimal
//            (Moffat-Katajainen in-place construction on symbols sorted by (count, symbol)), limited to 15 bits
//
// Kernels (all HBM traffic is one read of the planes, one write + one read of the scanlines, one write of the file):
//   png_filter_huff_kernel  one workgroup per deflate block: filter choice, scanlines, per-row Adler sums, histogram in
//                           LDS, code lengths + canonical codes (huff_code), bits of the block
//   png_emit_kernel         one workgroup per deflate block (emit_block): block start = sum of the previous blocks'
//                           bits; scanlines staged in LDS, per-thread bit counts, scan, bit packing (BitWriter: whole
//                           words stored, the two boundary words of a thread merged with atomicOr into the zeroed file)
//   (level 1: png_lz77_match_kernel + png_lz77_parse_kernel between these two, png_emit_lz77_kernel after the second;
//    see the level-1 section below)
//   png_trailer_kernel      container bytes, Adler-32 from the row sums
//   png_crc_kernel          CRC-32 of the IDAT chunk as XOR of 512-byte chunk CRCs multiplied by x^(8 * bytes behind)
//   png_crc_final_kernel    stores the CRC, the IEND chunk and the file size
// Shared by both levels, each written once: the block of a workgroup (block_ctx), the length-limited canonical code
// (huff_code), the block header (emit_block_header), the token codes (for_token_codes) and the bit packer (BitWriter).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <algorithm>
#include <cstring>
#include <new>

#include "../../include/ccd.h"

namespace {

constexpr int kMaxBits = 15;
constexpr int kHeaderBits = 3 + 5 + 5 + 4 + 19 * 3 + 258 * 4;  // 1106 bits in front of the first literal
constexpr int kBlockTarget = 32768;   // bytes of scanlines per deflate block (at least one row)
constexpr int kCrcChunk = 512;
constexpr int kDataStart = 43;        // signature 8 + IHDR 25 + IDAT length/type 8 + zlib header 2
constexpr int kMaxDim = 16383;        // 14-bit picture sizes (header.py:244-307); one scanline then fits the LDS stage
constexpr int kStageBytes = 49152;    // LDS stage of png_emit_kernel: >= max(kBlockTarget, 3 * kMaxDim + 1)
constexpr uint32_t kPoly = 0xEDB88320u;
constexpr int kNLL = 286, kNDist = 30;  // level 1: HLIT and HDIST of every LZ77 block

inline int rows_per_block(int w) { const int r = kBlockTarget / (3 * w + 1); return r < 1 ? 1 : r; }

constexpr int kMaxBatch = 64;        // pictures per launch set (a longer list is packed in several sets)

struct PngJob {                // one picture (a table of these lives in device memory)
    const uint8_t* plane[3];   // r, g, b: [h][w]
    uint32_t* out;             // the file, 4-byte aligned
    uint64_t cap_bits;
    uint8_t* scan;             // [h][3 w + 1] filtered scanlines
    uint32_t* codes;           // [nblk][257] bit-reversed code | length << 16
    uint32_t* blk_bits;        // [nblk]
    uint32_t* row_adler;       // [h][2] (sum d_i, sum (n - i) d_i) mod 65521
    uint32_t* meta;            // [0] deflate bits, [1] deflate bytes, [2] file bytes, [3] crc accumulator, [4] overflow flag
    int32_t h, w, rows, nblk;  // rows = rows per deflate block
    uint32_t zero_words, pad;  // words of `out` cleared before the bit packer merges into them
    // level 1 only (null at level 0), indexed like `scan` / per block
    uint16_t* prev;            // [h][3 w + 1] nearest earlier position of the block in the same bucket (kNone: none)
    uint32_t* lz;              // [h][3 w + 1] best match (length << 16 | distance), then the token starting there
    uint32_t* lz_codes;        // [nblk][kNLL + kNDist] bit-reversed code | length << 16
    uint32_t* lz_flag;         // [nblk] 1: the block is written with matches (png_emit_kernel leaves it alone)
};

struct PngBatch {              // kernel argument
    const PngJob* img;
    int32_t n, pad;
    uint32_t blk_prefix[kMaxBatch + 1];  // first workgroup of picture i in the per-block kernels
    uint32_t crc_prefix[kMaxBatch + 1];  // first workgroup of picture i in the CRC kernel
    uint32_t x2n[32];                    // x^(2^k) mod P (CRC-32, reflected)
};

// picture that owns workgroup `wg` (prefix[] sits in the kernel argument segment: scalar loads)
__device__ __forceinline__ int find_image(const uint32_t* prefix, int n, uint32_t wg) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= wg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the deflate block of this workgroup (the five per-block kernels run one workgroup per block of every picture)
struct BlockCtx {
    PngJob J;
    int k;           // block of the picture
    int N;           // bytes per scanline
    int y_lo, y_hi;  // rows of the block
    int nb;          // bytes of the block
    size_t off;      // first byte of the block in scan / prev / lz
};

__device__ __forceinline__ BlockCtx block_ctx(const PngBatch& B) {
    const int im = __builtin_amdgcn_readfirstlane(find_image(B.blk_prefix, B.n, blockIdx.x));
    BlockCtx C;
    C.J = B.img[im];
    C.k = static_cast<int>(blockIdx.x - B.blk_prefix[im]);
    C.N = 3 * C.J.w + 1;
    C.y_lo = C.k * C.J.rows;
    C.y_hi = min(C.J.h, C.y_lo + C.J.rows);
    C.nb = (C.y_hi - C.y_lo) * C.N;
    C.off = static_cast<size_t>(C.y_lo) * C.N;
    return C;
}

__device__ __forceinline__ int abs_res(int v) { v &= 255; return v < 128 ? v : 256 - v; }

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int filt_one(int f, int x, int a, int b, int c) {
    switch (f) {
        case 0: return x & 255;
        case 1: return (x - a) & 255;
        case 2: return (x - b) & 255;
        case 3: return (x - ((a + b) >> 1)) & 255;
        default: return (x - paeth(a, b, c)) & 255;
    }
}

__device__ __forceinline__ uint32_t rev_bits(uint32_t v, int n) { return __brev(v) >> (32 - n); }

// ---- length-limited canonical Huffman code over up to 512 symbols: the one construction of both levels ------------------
struct HuffLds {
    uint32_t key[512], A[512], par[512], dep[512], cnt[514];
    uint32_t num[kMaxBits + 1], first[kMaxBits + 1], base[kMaxBits + 1];
    uint32_t m;
};

// ascending sort of key[512] in LDS by the whole workgroup (behind a barrier that completes key; ends with one)
template <int kThreads>
__device__ __forceinline__ void bitonic_sort_512(uint32_t* key) {
    const int tid = threadIdx.x;
    for (int size = 2; size <= 512; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < 512; t += kThreads) {
                const int partner = t ^ stride;
                if (partner > t) {
                    const uint32_t a = key[t], b = key[partner];
                    const bool up = (t & size) == 0;
                    if ((a > b) == up) { key[t] = b; key[partner] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// hist[nsym] -> lens[nsym], codes[nsym] (bit-reversed code | length << 16).  Called by every thread of the workgroup,
// behind a barrier that completes hist; lens must be in LDS, codes may be anywhere.  The tree's depths take one
// internal node per thread: at most kThreads + 1 symbols may be used (level 0: 257 with 256 threads, exactly the limit).
template <int kThreads>
__device__ void huff_code(const uint32_t* hist, int nsym, uint32_t* lens, uint32_t* codes, HuffLds& S) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 514; i += kThreads) S.cnt[i] = 0;
    for (int i = tid; i < nsym; i += kThreads) lens[i] = 0;
    if (tid <= kMaxBits) S.num[tid] = 0;
    if (tid == 0) S.m = 0;
    __syncthreads();
    // ---- used symbols sorted by (count, symbol)
    for (int t = tid; t < 512; t += kThreads) {
        uint32_t key = 0xFFFFFFFFu;
        if (t < nsym && hist[t] > 0) { key = (hist[t] << 9) | static_cast<uint32_t>(t); atomicAdd(&S.m, 1u); }
        S.key[t] = key;
    }
    __syncthreads();
    bitonic_sort_512<kThreads>(S.key);
    const int m = static_cast<int>(S.m);
    if (m >= 2) {
        // ---- Huffman tree over the sorted symbols (one lane: the two-queue merge is sequential; at most 512 symbols).
        // Moffat-Katajainen phase 1, in place on the ascending counts: afterwards A[i] is the parent of internal node i.
        if (tid == 0) {
            uint32_t* A = S.A;
            for (int i = 0; i < m; ++i) A[i] = S.key[i] >> 9;
            A[0] += A[1];
            int root = 0, leaf = 2;
            for (int nxt = 1; nxt < m - 1; ++nxt) {
                if (leaf >= m || A[root] < A[leaf]) { A[nxt] = A[root]; A[root++] = nxt; }
                else A[nxt] = A[leaf++];
                if (leaf >= m || (root < nxt && A[root] < A[leaf])) { A[nxt] += A[root]; A[root++] = nxt; }
                else A[nxt] += A[leaf++];
            }
        }
        __syncthreads();
        // ---- depth of the internal nodes 0 .. m-2 (node m-2 is the root) by pointer jumping, one node per thread
        const int ni = m - 1;
        uint32_t par = 0, dep = 0;
        if (tid < ni) {
            par = tid == ni - 1 ? static_cast<uint32_t>(tid) : S.A[tid];
            dep = tid == ni - 1 ? 0u : 1u;
            S.par[tid] = par; S.dep[tid] = dep;
        }
        __syncthreads();
        for (int r = 0; r < 9; ++r) {  // 2^9 > 511 levels
            uint32_t pd = 0, pp = 0;
            if (tid < ni) { pd = S.dep[par]; pp = S.par[par]; }
            __syncthreads();
            if (tid < ni) { dep += pd; par = pp; S.dep[tid] = dep; S.par[tid] = par; }
            __syncthreads();
        }
        // ---- leaves per depth: the two children of every internal node at depth d - 1 are the internal nodes and the
        // leaves at depth d.  Sorted by count the leaves have non-increasing depths, so the counts per length are all
        // that is needed.  Limit to 15 bits: longer codes are folded into the limit here, the Kraft excess is worked
        // off below.
        if (tid < ni) atomicAdd(&S.cnt[dep], 1u);
        __syncthreads();
        for (int t = tid; t < 512; t += kThreads) {
            const int d = t + 1;
            const uint32_t leaves = 2u * S.cnt[d - 1] - S.cnt[d];
            if (leaves) atomicAdd(&S.num[min(d, kMaxBits)], leaves);
        }
        __syncthreads();
    } else if (tid == 0 && m == 1) {
        S.num[1] = 1;  // a single symbol: one code of length 1 (RFC 1951 allows an incomplete distance code)
    }
    if (tid == 0) {
        uint32_t total = 0;
        for (int l = 1; l <= kMaxBits; ++l) total += S.num[l] << (kMaxBits - l);
        while (m >= 2 && total != (1u << kMaxBits)) {
            S.num[kMaxBits]--;
            for (int l = kMaxBits - 1; l > 0; --l)
                if (S.num[l]) { S.num[l]--; S.num[l + 1] += 2; break; }
            --total;
        }
        // rarest symbols take the longest codes: sorted positions [first[l], first[l] + num[l]) get length l;
        // canonical codes (RFC 1951 3.2.2): first code of every length
        uint32_t first = 0, code = 0;
        for (int l = kMaxBits; l > 0; --l) { S.first[l] = first; first += S.num[l]; }
        for (int bits = 1; bits <= kMaxBits; ++bits) {
            code = (code + (bits > 1 ? S.num[bits - 1] : 0u)) << 1;
            S.base[bits] = code;
        }
    }
    __syncthreads();
    for (int j = tid; j < m; j += kThreads) {
        int l = kMaxBits;
        while (static_cast<uint32_t>(j) >= S.first[l] + S.num[l]) --l;
        lens[S.key[j] & 511u] = static_cast<uint32_t>(l);
    }
    __syncthreads();
    // ---- canonical codes: within a length, symbols in increasing order
    for (int sy = tid; sy < nsym; sy += kThreads) {
        const uint32_t l = lens[sy];
        uint32_t v = 0;
        if (l) {
            uint32_t rank = 0;
            for (int q = 0; q < sy; ++q) rank += lens[q] == l ? 1u : 0u;
            v = rev_bits(S.base[l] + rank, static_cast<int>(l)) | (l << 16);
        }
        codes[sy] = v;
    }
    __syncthreads();
}

// ---- kernel A -----------------------------------------------------------------------------------------------------
constexpr int kThreadsA = 256;   // 1024 threads: single pictures 10-20 % faster, batches and 4K 2x slower (occupancy; measured)

__global__ __launch_bounds__(kThreadsA) void png_filter_huff_kernel(PngBatch B) {
    __shared__ uint32_t s_hist[257];
    __shared__ uint32_t s_len[257];
    __shared__ unsigned long long s_red[kThreadsA / 64][8];
    __shared__ uint32_t s_sum;
    __shared__ HuffLds s_h;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const BlockCtx C = block_ctx(B);
    const PngJob& J = C.J;
    const int k = C.k, w = J.w, N = C.N;
    {   // this block's share of the file is cleared here (the bit packer of the next kernel merges into zeroed words)
        const uint32_t share = (J.zero_words + J.nblk - 1) / J.nblk;
        const uint32_t z_lo = min(J.zero_words, static_cast<uint32_t>(k) * share), z_hi = min(J.zero_words, z_lo + share);
        for (uint32_t i = z_lo + tid; i < z_hi; i += kThreadsA) J.out[i] = 0;
        if (k == 0 && tid < 8) J.meta[tid] = 0;
    }
    for (int i = tid; i < 257; i += kThreadsA) s_hist[i] = 0;
    if (tid == 0) s_sum = 0;
    __syncthreads();
    for (int y = C.y_lo; y < C.y_hi; ++y) {
        // ---- pass 1: cost of the five filters
        unsigned long long cost[5] = {0, 0, 0, 0, 0};
        for (int x = tid; x < w; x += kThreadsA) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint8_t* p = J.plane[c] + static_cast<size_t>(y) * w + x;
                const int cur = p[0];
                const int a = x > 0 ? p[-1] : 0;
                const int b = y > 0 ? p[-w] : 0;
                const int cc = (x > 0 && y > 0) ? p[-w - 1] : 0;
                cost[0] += abs_res(cur);
                cost[1] += abs_res(cur - a);
                cost[2] += abs_res(cur - b);
                cost[3] += abs_res(cur - ((a + b) >> 1));
                cost[4] += abs_res(cur - paeth(a, b, cc));
            }
        }
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            unsigned long long v = cost[f];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
            if (lane == 0) s_red[wave][f] = v;
        }
        __syncthreads();
        int ftype = 0;
        {
            unsigned long long best = ~0ull;
#pragma unroll
            for (int f = 0; f < 5; ++f) {
                unsigned long long v = 0;
                for (int q = 0; q < kThreadsA / 64; ++q) v += s_red[q][f];
                if (v < best) { best = v; ftype = f; }
            }
        }
        __syncthreads();
        // ---- pass 2: scanline, histogram, Adler sums
        uint8_t* row = J.scan + static_cast<size_t>(y) * N;
        unsigned long long sa = 0, sb = 0;
        if (tid == 0) {
            row[0] = static_cast<uint8_t>(ftype);
            atomicAdd(&s_hist[ftype], 1u);
            sa += ftype;
            sb += static_cast<unsigned long long>(N) * ftype;
        }
        for (int x = tid; x < w; x += kThreadsA) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint8_t* p = J.plane[c] + static_cast<size_t>(y) * w + x;
                const int cur = p[0];
                const int a = x > 0 ? p[-1] : 0;
                const int b = y > 0 ? p[-w] : 0;
                const int cc = (x > 0 && y > 0) ? p[-w - 1] : 0;
                const int v = filt_one(ftype, cur, a, b, cc);
                const int idx = 1 + 3 * x + c;
                row[idx] = static_cast<uint8_t>(v);
                atomicAdd(&s_hist[v], 1u);
                sa += v;
                sb += static_cast<unsigned long long>(N - idx) * v;
            }
        }
        for (int o = 32; o > 0; o >>= 1) { sa += __shfl_down(sa, o); sb += __shfl_down(sb, o); }
        if (lane == 0) { s_red[wave][5] = sa; s_red[wave][6] = sb; }
        __syncthreads();
        if (tid == 0) {
            unsigned long long ta = 0, tb = 0;
            for (int q = 0; q < kThreadsA / 64; ++q) { ta += s_red[q][5]; tb += s_red[q][6]; }
            J.row_adler[2 * y] = static_cast<uint32_t>(ta % 65521u);
            J.row_adler[2 * y + 1] = static_cast<uint32_t>(tb % 65521u);
        }
        __syncthreads();
    }
    // ---- code of the block's 257 symbols (a filter byte and end-of-block at least: never fewer than two used symbols)
    if (tid == 0) s_hist[256] = 1;
    __syncthreads();
    huff_code<kThreadsA>(s_hist, 257, s_len, J.codes + static_cast<size_t>(k) * 257, s_h);
    uint32_t part = 0;
    for (int sy = tid; sy < 257; sy += kThreadsA) part += s_hist[sy] * s_len[sy];
    atomicAdd(&s_sum, part);
    __syncthreads();
    if (tid == 0) J.blk_bits[k] = kHeaderBits + s_sum;
}

// ---- level 1: LZ77 inside each deflate block --------------------------------------------------------------------
// The canon (restated on the CPU by tests/png_lz77_ref.py):
//   match   position i of a block has a key if i + 2 < n; bucket h = ((b0 << 16 | b1 << 8 | b2) * 0x9E3779B1) >> 20.
//           Candidates: the kCand nearest earlier positions of the same bucket with i - j <= kWindow whose 3 bytes equal
//           those at i.  Length = common prefix (<= 258, <= end of the block, overlap allowed); best = longest, ties to
//           the nearest; < 3 is no match, length 3 farther than kFar3 is dropped.
//   parse   lazy-1: next(i) = i + L(i) if L(i) >= 3 and L(i + 1) <= L(i), else i + 1 (a literal).
//   code    dynamic Huffman, HLIT = 286, HDIST = 30, level 0's code-length code; both trees limited to 15 bits (the
//           construction of huff_code on up to 286 symbols; a single distance symbol gets length 1).
//   choice  a block whose exact bit count is not below its level-0 count keeps the level-0 coding (png_emit_kernel).
// Kernels, one workgroup per block, all between png_filter_huff_kernel and png_trailer_kernel (png_emit_kernel, the
// level-0 half of emit_block below, runs between the second and the third):
//   png_lz77_match_kernel  hash chains (prev[] in HBM scratch) and the best match of every position
//   png_lz77_parse_kernel  lazy parse by pointer jumping over next(i), histograms, both code constructions, exact bit
//                          counts, choice of the coding; the token of every position replaces its match
//   png_emit_lz77_kernel   emit_block for the blocks that take the matches: header, tokens, end-of-block
constexpr int kCand = 8;
constexpr int kWindow = 32768;
constexpr int kFar3 = 4096;
constexpr int kMaxMatch = 258;
constexpr int kBuckets = 4096;
constexpr uint16_t kNone = 0xFFFF;
constexpr int kHeaderBitsLz = 3 + 5 + 5 + 4 + 19 * 3 + (kNLL + kNDist) * 4;  // 1338

__device__ __forceinline__ uint32_t bucket3(uint32_t b0, uint32_t b1, uint32_t b2) {
    return ((b0 << 16 | b1 << 8 | b2) * 0x9E3779B1u) >> 20;
}

// length 3..258 -> symbol 257..285, extra bits, extra value
__device__ __forceinline__ void len_code(uint32_t L, uint32_t& sym, uint32_t& ne, uint32_t& ev) {
    if (L == kMaxMatch) { sym = 285; ne = 0; ev = 0; return; }
    const uint32_t x = L - 3;
    if (x < 8) { sym = 257 + x; ne = 0; ev = 0; return; }
    const uint32_t nb = 31 - __clz(x);
    sym = 257 + 4 * (nb - 1) + ((x >> (nb - 2)) & 3u);
    ne = nb - 2;
    ev = x & ((1u << ne) - 1);
}

// distance 1..32768 -> symbol 0..29, extra bits, extra value
__device__ __forceinline__ void dist_code(uint32_t D, uint32_t& sym, uint32_t& ne, uint32_t& ev) {
    const uint32_t x = D - 1;
    if (x < 4) { sym = x; ne = 0; ev = 0; return; }
    const uint32_t nb = 31 - __clz(x);
    sym = 2 * nb + ((x >> (nb - 1)) & 1u);
    ne = nb - 1;
    ev = x & ((1u << ne) - 1);
}

constexpr int kThreadsM = 256;
constexpr int kSegs = kThreadsM / 64;   // one segment of the block per wave while the chains are built

__global__ __launch_bounds__(kThreadsM) void png_lz77_match_kernel(PngBatch B) {
    __shared__ uint8_t s_data[kStageBytes];
    __shared__ uint16_t s_head[kSegs][kBuckets];  // last position of every bucket in the wave's segment so far
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const BlockCtx C = block_ctx(B);
    const PngJob& J = C.J;
    const int n = C.nb;
    const size_t off = C.off;
    uint16_t* prev = J.prev + off;
    uint32_t* mt = J.lz + off;
    for (int i = tid; i < n; i += kThreadsM) s_data[i] = J.scan[off + i];
    for (int i = tid; i < kSegs * kBuckets; i += kThreadsM) (&s_head[0][0])[i] = kNone;
    __syncthreads();
    // ---- chains inside the wave's segment, 64 positions per step: lanes of one bucket found with 12 ballots, the link
    // goes to the nearest earlier lane of the bucket, else to the segment's head; the last lane of a bucket moves the head
    const int seg = (n + 64 * kSegs - 1) / (64 * kSegs) * 64;
    const int s_lo = min(n, wave * seg), s_hi = min(n, s_lo + seg);
    for (int base = s_lo; base < s_hi; base += 64) {
        const int i = base + lane;
        const bool valid = i < s_hi && i + 2 < n;
        const uint32_t h = valid ? bucket3(s_data[i], s_data[i + 1], s_data[i + 2]) : 0u;
        uint64_t same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 12; ++b) {
            const bool bit = (h >> b) & 1u;
            const uint64_t bal = __ballot(valid && bit);
            same &= bit ? bal : ~bal;
        }
        if (valid) {
            const uint64_t below = same & ((1ull << lane) - 1);
            const uint64_t above = same & ~((2ull << lane) - 1);
            prev[i] = below ? static_cast<uint16_t>(base + 63 - __clzll(below)) : s_head[wave][h];
            if (!above) s_head[wave][h] = static_cast<uint16_t>(i);
        }
    }
    __syncthreads();
    // ---- the first position of a bucket in a segment links to the last one in the segments before (same lanes as above)
    for (int i = s_lo + lane; i < s_hi; i += 64) {
        if (i + 2 >= n || prev[i] != kNone) continue;
        const uint32_t h = bucket3(s_data[i], s_data[i + 1], s_data[i + 2]);
        uint16_t p = kNone;
        for (int s = wave - 1; s >= 0 && p == kNone; --s) p = s_head[s][h];
        prev[i] = p;
    }
    __syncthreads();
    // ---- best match of every position: at most kCand links, lengths compared in LDS
    for (int i = tid; i < n; i += kThreadsM) {
        uint32_t res = 0;
        if (i + 2 < n) {
            const uint8_t c0 = s_data[i], c1 = s_data[i + 1], c2 = s_data[i + 2];
            const int lim = min(kMaxMatch, n - i);
            int best = 0, bd = 0;
            uint32_t j = prev[i];
            for (int t = 0; t < kCand && j != kNone && i - static_cast<int>(j) <= kWindow; ++t) {
                if (s_data[j] == c0 && s_data[j + 1] == c1 && s_data[j + 2] == c2) {
                    int l = 3;
                    while (l < lim && s_data[j + l] == s_data[i + l]) ++l;
                    if (l > best) { best = l; bd = i - static_cast<int>(j); }
                    if (best == lim) break;  // nothing longer exists; ties stay with the nearer candidate
                }
                j = prev[j];
            }
            if (best >= 3 && !(best == 3 && bd > kFar3)) res = (static_cast<uint32_t>(best) << 16) | static_cast<uint32_t>(bd);
        }
        mt[i] = res;
    }
}

constexpr int kThreadsP = 1024;
constexpr int kPerThreadP = kStageBytes / kThreadsP;  // positions per thread in the pointer jumping (48, in 24 pairs)
constexpr int kJumpRounds = 16;                       // 2^16 > kStageBytes steps of next()

__global__ __launch_bounds__(kThreadsP) void png_lz77_parse_kernel(PngBatch B) {
    __shared__ uint32_t s_next2[kStageBytes / 2 + 1];  // next^(2^r)(i) as u16, two per word; n is the end
    uint16_t* s_next = reinterpret_cast<uint16_t*>(s_next2);
    __shared__ uint32_t s_mark[kStageBytes / 32];  // token starts found so far
    __shared__ uint32_t s_take[kStageBytes / 32];  // a token starting here is the match found there
    __shared__ uint32_t s_hll[kNLL], s_hd[kNDist], s_len[kNLL + kNDist], s_code[kNLL + kNDist];
    __shared__ HuffLds s_h;
    __shared__ uint32_t s_bits, s_lit_bits;  // bits of the LZ77 coding; of the level-0 coding (png_filter_huff_kernel)
    const int tid = threadIdx.x;
    const BlockCtx C = block_ctx(B);
    const PngJob& J = C.J;
    const int k = C.k, n = C.nb;
    const size_t off = C.off;
    uint32_t* mt = J.lz + off;
    for (int i = tid; i < kStageBytes / 32; i += kThreadsP) { s_mark[i] = i == 0 ? 1u : 0u; s_take[i] = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += kThreadsP) {
        const uint32_t L = mt[i] >> 16, L1 = i + 1 < n ? mt[i + 1] >> 16 : 0u;
        const bool take = L >= 3 && L1 <= L;
        s_next[i] = static_cast<uint16_t>(take ? i + static_cast<int>(L) : i + 1);
        if (take) atomicOr(&s_take[i >> 5], 1u << (i & 31));
    }
    if (tid == 0) {
        s_next[n] = s_next[n + 1] = static_cast<uint16_t>(n);  // n + 1 shares the last pair word (n <= kStageBytes - 2)
        s_bits = 0;
        s_lit_bits = J.blk_bits[k];
    }
    for (int i = tid; i < kNLL; i += kThreadsP) s_hll[i] = i == 256 ? 1u : 0u;
    for (int i = tid; i < kNDist; i += kThreadsP) s_hd[i] = 0;
    __syncthreads();
    // ---- token starts = the path from 0.  Round r: every marked i marks next^(2^r)(i), then the jump doubles.  After
    // round r the first 2^(r+1) steps of the path are marked (a mark set early in a round only adds path positions).
    // Each thread owns the position pairs (2 p, 2 p + 1), p = tid + q * kThreadsP: one LDS word per pair and per round.
    // Positions >= n keep jumping to n (s_next[n] = n, and the pair word of n - 1 / n is read and written whole).
    const int pairs = (n + 2) / 2;  // words of s_next that hold positions 0 .. n
    for (int r = 0; r < kJumpRounds; ++r) {
        uint32_t nn[kPerThreadP / 2];  // the pair's two new jumps
#pragma unroll
        for (int q = 0; q < kPerThreadP / 2; ++q) {
            const int p = tid + q * kThreadsP;
            uint32_t v = 0;
            if (p < pairs) {
                const uint32_t w = s_next2[p];
                const uint32_t mk = (s_mark[p >> 4] >> ((2 * p) & 31)) & 3u;
                const int j0 = static_cast<int>(w & 0xFFFFu), j1 = static_cast<int>(w >> 16);
                if ((mk & 1u) && j0 < n) atomicOr(&s_mark[j0 >> 5], 1u << (j0 & 31));
                if ((mk & 2u) && j1 < n) atomicOr(&s_mark[j1 >> 5], 1u << (j1 & 31));
                v = static_cast<uint32_t>(s_next[j0]) | (static_cast<uint32_t>(s_next[j1]) << 16);
            }
            nn[q] = v;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPerThreadP / 2; ++q) {
            const int p = tid + q * kThreadsP;
            if (p < pairs) s_next2[p] = nn[q];
        }
        __syncthreads();
        if (s_next[0] == n) break;  // the path from 0 ends within the 2^(r+1) steps marked so far
    }
    // ---- tokens (0: inside a match, 1: a literal, else the match), histograms, extra bits
    uint32_t extra = 0;
    for (int i = tid; i < n; i += kThreadsP) {
        uint32_t tok = 0;
        if ((s_mark[i >> 5] >> (i & 31)) & 1u) {
            if ((s_take[i >> 5] >> (i & 31)) & 1u) {
                tok = mt[i];
                uint32_t sym, ne, ev;
                len_code(tok >> 16, sym, ne, ev);
                atomicAdd(&s_hll[sym], 1u);
                extra += ne;
                dist_code(tok & 0xFFFFu, sym, ne, ev);
                atomicAdd(&s_hd[sym], 1u);
                extra += ne;
            } else {
                atomicAdd(&s_hll[J.scan[off + i]], 1u);
                tok = 1;
            }
        }
        mt[i] = tok;
    }
    atomicAdd(&s_bits, extra);
    __syncthreads();
    huff_code<kThreadsP>(s_hll, kNLL, s_len, s_code, s_h);
    huff_code<kThreadsP>(s_hd, kNDist, s_len + kNLL, s_code + kNLL, s_h);
    uint32_t part = 0;
    for (int s = tid; s < kNLL + kNDist; s += kThreadsP) part += (s < kNLL ? s_hll[s] : s_hd[s - kNLL]) * s_len[s];
    atomicAdd(&s_bits, part);
    __syncthreads();
    const uint32_t bits = kHeaderBitsLz + s_bits;
    // every thread decides from LDS: thread 0 alone reads blk_bits[k] (at the start) and writes it (below)
    const bool lz = bits < s_lit_bits;  // else the level-0 coding of png_filter_huff_kernel stays
    if (lz) for (int s = tid; s < kNLL + kNDist; s += kThreadsP) J.lz_codes[static_cast<size_t>(k) * (kNLL + kNDist) + s] = s_code[s];
    if (tid == 0) {
        J.lz_flag[k] = lz ? 1u : 0u;
        if (lz) J.blk_bits[k] = bits;
    }
}

// ---- kernel B: the bits of a block, both levels -------------------------------------------------------------------
constexpr int kThreadsB = 256;

// merges the low nbits of value into the zeroed file at bit pos (any thread, any position)
__device__ __forceinline__ void or_bits(uint32_t* out, uint64_t pos, uint32_t value, int nbits) {
    if (nbits == 0) return;
    const uint64_t v = static_cast<uint64_t>(value) << (pos & 31);
    atomicOr(&out[pos >> 5], static_cast<uint32_t>(v));
    if ((pos & 31) + nbits > 32) atomicOr(&out[(pos >> 5) + 1], static_cast<uint32_t>(v >> 32));
}

// Bits of the deflate stream in front of block k = bits of all blocks before it.  Called by every thread; its barrier
// also publishes what the caller staged in LDS before the call.
__device__ __forceinline__ unsigned long long block_start_bits(const PngJob& J, int k, unsigned long long* s_part) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned long long before = 0;
    for (int i = tid; i < k; i += kThreadsB) before += J.blk_bits[i];
    for (int o = 32; o > 0; o >>= 1) before += __shfl_down(before, o);
    if (lane == 0) s_part[wave] = before;
    __syncthreads();
    before = 0;
    for (int q = 0; q < kThreadsB / 64; ++q) before += s_part[q];
    return before;
}

// Header of a dynamic-Huffman block at bit `start`: BFINAL, BTYPE = 2, HLIT, HDIST, HCLEN = 19; the code-length code
// (3-bit lengths in the order 16, 17, 18, 0, 8, ...: none for the run-length symbols, 4 bits for each of the lengths
// 0..15); the hlit + hdist lengths, 4 bits each (those of code[n_codes], zero behind them).  The end-of-block code goes
// in front of bit `end`, the first bit behind the block.
__device__ __forceinline__ void emit_block_header(uint32_t* out, uint64_t start, uint64_t end, bool final_blk, uint32_t hlit,
                                                  uint32_t hdist, const uint32_t* code, int n_codes) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        or_bits(out, start, (final_blk ? 1u : 0u) | (2u << 1) | ((hlit - 257u) << 3) | ((hdist - 1u) << 8) | (15u << 13), 17);
        const uint32_t eob = code[256];
        or_bits(out, end - (eob >> 16), eob & 0xFFFFu, static_cast<int>(eob >> 16));
    }
    if (tid < 19) or_bits(out, start + 17 + 3 * tid, tid < 3 ? 0u : 4u, 3);
    for (int s = tid; s < static_cast<int>(hlit + hdist); s += kThreadsB)
        or_bits(out, start + 74 + 4 * s, rev_bits(s < n_codes ? code[s] >> 16 : 0u, 4), 4);
}

// exclusive scan of one value per thread over the workgroup (s_scan: one word per wave; holds a barrier)
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t* s_scan) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_scan[wave] = incl;
    __syncthreads();
    uint32_t offset = incl - v;
    for (int q = 0; q < wave; ++q) offset += s_scan[q];
    return offset;
}

// Packs the consecutive codes of one thread into the zeroed file from bit `pos` on.  The one place that decides how an
// output word is written: the first word a thread completes and its last, partial word may hold bits of its
// neighbours and are merged with atomicOr; every bit of a word between them belongs to this thread, which stores it.
struct BitWriter {
    uint32_t* out;
    uint32_t wi;
    int nacc;
    uint64_t acc = 0;
    bool first = true;
    __device__ BitWriter(uint32_t* o, uint64_t pos) : out(o), wi(static_cast<uint32_t>(pos >> 5)), nacc(static_cast<int>(pos & 31)) {}
    __device__ void put(uint32_t value, int n) {  // n <= 15
        acc |= static_cast<uint64_t>(value) << nacc;
        nacc += n;
        if (nacc >= 32) {
            if (first) atomicOr(&out[wi], static_cast<uint32_t>(acc));
            else out[wi] = static_cast<uint32_t>(acc);
            first = false;
            ++wi;
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ void flush() {
        if (nacc > 0 && acc != 0) atomicOr(&out[wi], static_cast<uint32_t>(acc));
    }
};

// The codes of the token that starts at position i of the block, in stream order, as put(value, nbits).  Level 0: every
// position is a literal.  Level 1: tk[i] is 0 inside a match, 1 for a literal, else length << 16 | distance.
template <bool LZ, typename Put>
__device__ __forceinline__ void for_token_codes(const uint32_t* tk, const uint8_t* data, const uint32_t* code, int i, Put&& put) {
    const uint32_t t = LZ ? tk[i] : 1u;
    if (!t) return;
    if (t >> 16) {
        const uint32_t* dcode = code + kNLL;
        uint32_t sym, ne, ev;
        len_code(t >> 16, sym, ne, ev);
        put(code[sym] & 0xFFFFu, static_cast<int>(code[sym] >> 16));
        put(ev, static_cast<int>(ne));
        dist_code(t & 0xFFFFu, sym, ne, ev);
        put(dcode[sym] & 0xFFFFu, static_cast<int>(dcode[sym] >> 16));
        put(ev, static_cast<int>(ne));
    } else {
        const uint32_t c = code[data[i]];
        put(c & 0xFFFFu, static_cast<int>(c >> 16));
    }
}

// One workgroup writes one block.  Level 0 (png_emit_kernel) runs for every block, keeps the stream's bit count and the
// overflow flag, and leaves the blocks that png_lz77_parse_kernel flagged to level 1 (png_emit_lz77_kernel), which
// writes those alone.
template <bool LZ>
__device__ __forceinline__ void emit_block(const PngBatch& B) {
    constexpr int kCodes = LZ ? kNLL + kNDist : 257;
    __shared__ uint8_t s_data[kStageBytes];
    __shared__ uint32_t s_code[kCodes];
    __shared__ unsigned long long s_part[kThreadsB / 64];
    __shared__ uint32_t s_scan[kThreadsB / 64];
    const int tid = threadIdx.x;
    const BlockCtx C = block_ctx(B);
    const PngJob& J = C.J;
    const int k = C.k, nb = C.nb;
    if (LZ && !J.lz_flag[k]) return;
    const uint32_t* codes = (LZ ? J.lz_codes : J.codes) + static_cast<size_t>(k) * kCodes;
    for (int i = tid; i < kCodes; i += kThreadsB) s_code[i] = codes[i];
    for (int i = tid; i < nb; i += kThreadsB) s_data[i] = J.scan[C.off + i];
    const unsigned long long before = block_start_bits(J, k, s_part);  // the barrier behind s_code and s_data
    const uint32_t my_bits = J.blk_bits[k];
    const uint64_t start = static_cast<uint64_t>(kDataStart) * 8 + before;
    if (!LZ && k == J.nblk - 1 && tid == 0) J.meta[0] = static_cast<uint32_t>(before + my_bits);
    if (start + my_bits + 256 > J.cap_bits) {  // 20 container bytes follow the last block
        if (!LZ && tid == 0) J.meta[4] = 1;    // never with a buffer of ccd_png_bound() bytes
        return;
    }
    if (!LZ && J.lz_flag && J.lz_flag[k]) return;
    emit_block_header(J.out, start, start + my_bits, k == J.nblk - 1, LZ ? kNLL : 257, LZ ? kNDist : 1, s_code, kCodes);
    // ---- tokens starting in a contiguous chunk of positions per thread: bit counts, scan, packing
    const uint32_t* tk = LZ ? J.lz + C.off : nullptr;
    const int cb = (nb + kThreadsB - 1) / kThreadsB;
    const int lo = min(nb, tid * cb), hi = min(nb, lo + cb);
    uint32_t bits = 0;
    for (int i = lo; i < hi; ++i) for_token_codes<LZ>(tk, s_data, s_code, i, [&](uint32_t, int n) { bits += n; });
    BitWriter bw(J.out, start + (LZ ? kHeaderBitsLz : kHeaderBits) + wg_exclusive_scan(bits, s_scan));
    for (int i = lo; i < hi; ++i) for_token_codes<LZ>(tk, s_data, s_code, i, [&](uint32_t v, int n) { bw.put(v, n); });
    bw.flush();
}

__global__ __launch_bounds__(kThreadsB) void png_emit_kernel(PngBatch B) { emit_block<false>(B); }

__global__ __launch_bounds__(kThreadsB) void png_emit_lz77_kernel(PngBatch B) { emit_block<true>(B); }

// ---- kernel C -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
    p[0] = static_cast<uint8_t>(v >> 24); p[1] = static_cast<uint8_t>(v >> 16);
    p[2] = static_cast<uint8_t>(v >> 8); p[3] = static_cast<uint8_t>(v);
}

__global__ __launch_bounds__(256) void png_trailer_kernel(PngBatch B) {
    __shared__ unsigned long long s_r[4][3];
    const PngJob J = B.img[blockIdx.x];
    if (J.meta[4]) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // Adler-32 of the scanlines from the row sums.  Row after row it is B += N A + b_r, A += a_r, starting at A = 1, B = 0;
    // in closed form A = 1 + sum a_q and B = sum b_q + N (H + sum a_q (H - 1 - q)), everything modulo 65521.
    unsigned long long sa = 0, sb = 0, sw = 0;
    for (int q = tid; q < J.h; q += 256) {
        const unsigned long long a = J.row_adler[2 * q];
        sa += a;
        sb += J.row_adler[2 * q + 1];
        sw += a * static_cast<unsigned long long>(J.h - 1 - q);  // < 2^16 * 2^14 per term, at most 64 terms per thread
    }
    for (int o = 32; o > 0; o >>= 1) { sa += __shfl_down(sa, o); sb += __shfl_down(sb, o); sw += __shfl_down(sw, o); }
    if (lane == 0) { s_r[wave][0] = sa; s_r[wave][1] = sb; s_r[wave][2] = sw; }
    __syncthreads();
    if (tid != 0) return;
    sa = sb = sw = 0;
    for (int q = 0; q < 4; ++q) { sa += s_r[q][0]; sb += s_r[q][1]; sw += s_r[q][2]; }
    const unsigned long long M = 65521ull, N = static_cast<unsigned long long>(3 * J.w + 1) % M;
    const uint32_t ad_a = static_cast<uint32_t>((1 + sa) % M);
    const uint32_t ad_b = static_cast<uint32_t>((sb % M + N * ((static_cast<unsigned long long>(J.h) + sw % M) % M)) % M);
    uint8_t* out = reinterpret_cast<uint8_t*>(J.out);
    const uint32_t n_def = (J.meta[0] + 7u) >> 3;
    J.meta[1] = n_def;
    // signature, IHDR (8-bit RGB, deflate, adaptive filtering, no interlace), IDAT type, zlib header (32 KB window, no
    // preset dictionary, check bits).  Bytes 40..42 share a word with the first deflate byte, which is already there.
    uint8_t head[kDataStart];
    for (int i = 0; i < kDataStart; ++i) head[i] = 0;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    for (int i = 0; i < 8; ++i) head[i] = sig[i];
    head[11] = 13;
    head[12] = 'I'; head[13] = 'H'; head[14] = 'D'; head[15] = 'R';
    put_be32(head + 16, static_cast<uint32_t>(J.w));
    put_be32(head + 20, static_cast<uint32_t>(J.h));
    head[24] = 8; head[25] = 2;
    {
        uint32_t crc = 0xFFFFFFFFu;
        for (int i = 12; i < 29; ++i) {
            crc ^= head[i];
            for (int b = 0; b < 8; ++b) crc = (crc & 1u) ? (crc >> 1) ^ kPoly : crc >> 1;
        }
        put_be32(head + 29, crc ^ 0xFFFFFFFFu);
    }
    head[37] = 'I'; head[38] = 'D'; head[39] = 'A'; head[40] = 'T'; head[41] = 0x78; head[42] = 0x01;
    for (int i = 0; i < 40; ++i) out[i] = head[i];
    for (int i = 40; i < kDataStart; ++i) out[i] |= head[i];
    put_be32(out + 33, 2u + n_def + 4u);
    put_be32(out + kDataStart + n_def, (ad_b << 16) | ad_a);
}

// ---- kernel D -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}

__global__ __launch_bounds__(256) void png_crc_kernel(PngBatch B) {
    // slice-by-4 tables: s_tab[j][v] = CRC of byte v followed by j zero bytes
    __shared__ uint32_t s_tab[4][256];
    {
        uint32_t c = threadIdx.x;
        for (int i = 0; i < 8; ++i) c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
        s_tab[0][threadIdx.x] = c;
    }
    __syncthreads();
    for (int j = 1; j < 4; ++j) {
        const uint32_t c = s_tab[j - 1][threadIdx.x];
        s_tab[j][threadIdx.x] = (c >> 8) ^ s_tab[0][c & 255u];
        __syncthreads();
    }
    const int im = __builtin_amdgcn_readfirstlane(find_image(B.crc_prefix, B.n, blockIdx.x));
    const PngJob J = B.img[im];
    if (J.meta[4]) return;
    // The IDAT chunk's CRC covers its type and data: file bytes [37, end).  Chunks are cut at multiples of kCrcChunk of
    // the FILE offset, so every chunk but the first starts on a word.
    const uint64_t end = 37ull + 4ull + 2ull + J.meta[1] + 4ull;
    const uint64_t c0 = (static_cast<uint64_t>(blockIdx.x - B.crc_prefix[im]) * 256 + threadIdx.x) * kCrcChunk;
    uint32_t part = 0;  // this chunk's term of the file CRC
    if (c0 < end) {
        uint64_t i = c0 < 37 ? 37 : c0;
        const uint64_t hi = min(end, c0 + kCrcChunk);
        const uint8_t* p = reinterpret_cast<const uint8_t*>(J.out);
        uint32_t crc = 0xFFFFFFFFu;
        for (; i < hi && (i & 3); ++i) crc = s_tab[0][(crc ^ p[i]) & 255u] ^ (crc >> 8);
        for (; i + 4 <= hi; i += 4) {
            crc ^= J.out[i >> 2];
            crc = s_tab[3][crc & 255u] ^ s_tab[2][(crc >> 8) & 255u] ^ s_tab[1][(crc >> 16) & 255u] ^ s_tab[0][crc >> 24];
        }
        for (; i < hi; ++i) crc = s_tab[0][(crc ^ p[i]) & 255u] ^ (crc >> 8);
        crc ^= 0xFFFFFFFFu;
        // multiply by x^(8 * bytes behind the chunk)
        uint64_t behind = end - hi;
        uint32_t xp = 1u << 31;
        for (int kbit = 3; behind; behind >>= 1, ++kbit)
            if (behind & 1) xp = multmodp(B.x2n[kbit & 31], xp);
        part = multmodp(xp, crc);
    }
    // one atomic per wave (tens of thousands of chunks otherwise queue up on one address)
    for (int o = 32; o > 0; o >>= 1) part ^= __shfl_xor(part, o);
    if ((threadIdx.x & 63) == 0 && part) atomicXor(&J.meta[3], part);
}

__global__ void png_crc_final_kernel(PngBatch B) {
    const PngJob J = B.img[blockIdx.x];
    if (threadIdx.x != 0 || J.meta[4]) return;
    uint8_t* out = reinterpret_cast<uint8_t*>(J.out);
    const uint32_t n_def = J.meta[1];
    uint8_t* p = out + kDataStart + n_def + 4;
    put_be32(p, J.meta[3]);
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) p[4 + i] = iend[i];
    J.meta[2] = kDataStart + n_def + 4 + 4 + 12;
}

// ---- host side ----------------------------------------------------------------------------------------------------
uint32_t host_multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}

template <typename T>
bool grow(T** buf, size_t* cap, size_t need) {  // device buffer of at least `need` elements (contents are scratch)
    if (need <= *cap) return true;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(buf), need * sizeof(T)) != hipSuccess) return false;
    *cap = need;
    return true;
}

template <typename T>
bool regrow_pinned(T** buf, size_t need) {  // pinned host buffer of `need` elements (contents are scratch)
    if (*buf) (void)hipHostFree(*buf);
    *buf = nullptr;
    return hipHostMalloc(reinterpret_cast<void**>(buf), need * sizeof(T), hipHostMallocDefault) == hipSuccess;
}

// bytes of a picture's scanlines in the workspace (every picture starts on a multiple of 16)
inline size_t scan_bytes(int h, int w) { return (static_cast<size_t>(h) * (3 * static_cast<size_t>(w) + 1) + 15) & ~static_cast<size_t>(15); }

}  // namespace

struct ccd_png {
    int device = 0;
    size_t scan_cap = 0, codes_cap = 0, bits_cap = 0, adler_cap = 0, jobs_cap = 0, meta_cap = 0;
    uint8_t* d_scan = nullptr;
    uint32_t* d_codes = nullptr;     // [blocks][257]
    uint32_t* d_blk_bits = nullptr;  // [blocks]
    uint32_t* d_row_adler = nullptr; // [rows][2]
    uint32_t* d_meta = nullptr;      // [pictures][8]
    uint32_t* h_meta = nullptr;      // pinned copy of d_meta
    // job table: two pinned host copies and two device copies used alternately, each guarded by an event recorded behind the
    // kernels that read it - a pack neither blocks on the stream nor hands the runtime a pageable buffer
    PngJob* d_jobs[2] = {nullptr, nullptr};
    PngJob* h_jobs[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ev_used[2] = {false, false};
    int flip = 0;
    uint32_t x2n[32];
    int pending = 0;                 // pictures of the pack in flight
    hipStream_t pack_stream = nullptr;  // ... and the stream it was enqueued on
    int level = CCD_PNG_LITERAL;     // read when a pack is enqueued
    // level 1 workspace
    size_t prev_cap = 0, lz_cap = 0, lzc_cap = 0, flag_cap = 0;
    uint16_t* d_prev = nullptr;      // [scan bytes]
    uint32_t* d_lz = nullptr;        // [scan bytes]
    uint32_t* d_lz_codes = nullptr;  // [blocks][kNLL + kNDist]
    uint32_t* d_lz_flag = nullptr;   // [blocks]
};

namespace {

struct PackSize { size_t scan = 0, blocks = 0, rows = 0; };  // of all pictures of a pack: scanline bytes, deflate blocks, rows

bool validate_and_size(const ccd_png_item* items, int n, PackSize* sz) {
    for (int i = 0; i < n; ++i) {
        const ccd_png_item& it = items[i];
        if (!it.r || !it.g || !it.b || !it.out || it.h <= 0 || it.w <= 0 || it.h > kMaxDim || it.w > kMaxDim) return false;
        if ((reinterpret_cast<uintptr_t>(it.out) & 3u) || it.cap < ccd_png_bound(it.h, it.w)) return false;
        const int rpb = rows_per_block(it.w);
        sz->scan += scan_bytes(it.h, it.w);
        sz->blocks += (it.h + rpb - 1) / rpb;
        sz->rows += it.h;
    }
    return true;
}

// Workspace for a pack of n pictures.  Before a buffer is replaced the stream is drained: the previous pack may still use it.
int ensure_workspace(ccd_png* p, int n, const PackSize& sz, bool lz, hipStream_t st) {
    const size_t pics = static_cast<size_t>(n), lz_codes = sz.blocks * (kNLL + kNDist);
    if (lz && (sz.scan > p->prev_cap || sz.scan > p->lz_cap || lz_codes > p->lzc_cap || sz.blocks > p->flag_cap)) {
        if (hipStreamSynchronize(st) != hipSuccess) return CCD_ERR_HIP;
        if (!grow(&p->d_prev, &p->prev_cap, sz.scan) || !grow(&p->d_lz, &p->lz_cap, sz.scan) ||
            !grow(&p->d_lz_codes, &p->lzc_cap, lz_codes) || !grow(&p->d_lz_flag, &p->flag_cap, sz.blocks))
            return CCD_ERR_NOMEM;
    }
    if (sz.scan > p->scan_cap || sz.blocks * 257 > p->codes_cap || sz.blocks > p->bits_cap || sz.rows * 2 > p->adler_cap ||
        pics > p->jobs_cap || pics * 8 > p->meta_cap) {
        if (hipStreamSynchronize(st) != hipSuccess) return CCD_ERR_HIP;
        if (pics * 8 > p->meta_cap && !regrow_pinned(&p->h_meta, pics * 8)) return CCD_ERR_NOMEM;
        if (!grow(&p->d_scan, &p->scan_cap, sz.scan) || !grow(&p->d_codes, &p->codes_cap, sz.blocks * 257) ||
            !grow(&p->d_blk_bits, &p->bits_cap, sz.blocks) || !grow(&p->d_row_adler, &p->adler_cap, sz.rows * 2) ||
            !grow(&p->d_meta, &p->meta_cap, pics * 8))
            return CCD_ERR_NOMEM;
        if (pics > p->jobs_cap) {
            for (int k = 0; k < 2; ++k) {
                size_t cap = p->jobs_cap;
                if (!grow(&p->d_jobs[k], &cap, pics) || !regrow_pinned(&p->h_jobs[k], pics)) return CCD_ERR_NOMEM;
                if (!p->ev[k] && hipEventCreateWithFlags(&p->ev[k], hipEventDisableTiming) != hipSuccess) return CCD_ERR_HIP;
                p->ev_used[k] = false;  // the stream was drained above
            }
            p->jobs_cap = pics;
        }
    }
    return CCD_OK;
}

// the job table of a pack: every picture gets its slice of each workspace buffer
void fill_jobs(const ccd_png* p, PngJob* jobs, const ccd_png_item* items, int n, bool lz) {
    size_t scan_off = 0, blk_off = 0, row_off = 0;
    for (int i = 0; i < n; ++i) {
        const ccd_png_item& it = items[i];
        PngJob& J = jobs[i];
        std::memset(&J, 0, sizeof(J));
        J.plane[0] = it.r; J.plane[1] = it.g; J.plane[2] = it.b;
        J.out = reinterpret_cast<uint32_t*>(it.out);
        J.cap_bits = static_cast<uint64_t>(it.cap) * 8;
        J.h = it.h; J.w = it.w; J.rows = rows_per_block(it.w); J.nblk = (it.h + J.rows - 1) / J.rows;
        J.scan = p->d_scan + scan_off;
        J.codes = p->d_codes + blk_off * 257;
        J.blk_bits = p->d_blk_bits + blk_off;
        J.row_adler = p->d_row_adler + row_off * 2;
        J.meta = p->d_meta + static_cast<size_t>(i) * 8;
        if (lz) {
            J.prev = p->d_prev + scan_off;
            J.lz = p->d_lz + scan_off;
            J.lz_codes = p->d_lz_codes + blk_off * (kNLL + kNDist);
            J.lz_flag = p->d_lz_flag + blk_off;
        }
        const size_t bound = ccd_png_bound(it.h, it.w);
        J.zero_words = static_cast<uint32_t>(std::min(it.cap & ~static_cast<size_t>(3), (bound + 3) & ~static_cast<size_t>(3)) / 4);
        scan_off += scan_bytes(it.h, it.w);
        blk_off += J.nblk;
        row_off += it.h;
    }
}

// one set of launches for cnt <= kMaxBatch pictures (jobs: their entries of the host table, d_jobs: of the device table)
int launch_set(const ccd_png* p, const PngJob* jobs, const PngJob* d_jobs, int cnt, bool lz, hipStream_t st) {
    PngBatch B;
    std::memset(&B, 0, sizeof(B));
    B.img = d_jobs;
    B.n = cnt;
    std::memcpy(B.x2n, p->x2n, sizeof(B.x2n));
    for (int i = 0; i < cnt; ++i) {
        B.blk_prefix[i + 1] = B.blk_prefix[i] + static_cast<uint32_t>(jobs[i].nblk);
        const size_t chunks = ccd_png_bound(jobs[i].h, jobs[i].w) / kCrcChunk + 1;
        B.crc_prefix[i + 1] = B.crc_prefix[i] + static_cast<uint32_t>((chunks + 255) / 256);
    }
    const dim3 blocks(B.blk_prefix[cnt]);
    hipLaunchKernelGGL(png_filter_huff_kernel, blocks, dim3(kThreadsA), 0, st, B);
    if (lz) {
        hipLaunchKernelGGL(png_lz77_match_kernel, blocks, dim3(kThreadsM), 0, st, B);
        hipLaunchKernelGGL(png_lz77_parse_kernel, blocks, dim3(kThreadsP), 0, st, B);
    }
    hipLaunchKernelGGL(png_emit_kernel, blocks, dim3(kThreadsB), 0, st, B);
    if (lz) hipLaunchKernelGGL(png_emit_lz77_kernel, blocks, dim3(kThreadsB), 0, st, B);
    hipLaunchKernelGGL(png_trailer_kernel, dim3(cnt), dim3(256), 0, st, B);
    hipLaunchKernelGGL(png_crc_kernel, dim3(B.crc_prefix[cnt]), dim3(256), 0, st, B);
    hipLaunchKernelGGL(png_crc_final_kernel, dim3(cnt), dim3(64), 0, st, B);
    return hipGetLastError() == hipSuccess ? CCD_OK : CCD_ERR_HIP;
}

}  // namespace

extern "C" {

size_t ccd_png_bound(int h, int w) {
    if (h <= 0 || w <= 0 || h > kMaxDim || w > kMaxDim) return 0;
    const size_t raw = static_cast<size_t>(h) * (3 * static_cast<size_t>(w) + 1);
    const size_t nblk = (static_cast<size_t>(h) + rows_per_block(w) - 1) / rows_per_block(w);
    return (raw * 10 + 7) / 8 + nblk * 144 + 128;
}

int ccd_png_create(int device, ccd_png** out) {
    if (!out) return CCD_ERR_ARG;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return CCD_ERR_HIP;
    ccd_png* p = new (std::nothrow) ccd_png();
    if (!p) return CCD_ERR_NOMEM;
    p->device = device;
    p->x2n[0] = 1u << 30;
    for (int k = 1; k < 32; ++k) p->x2n[k] = host_multmodp(p->x2n[k - 1], p->x2n[k - 1]);
    *out = p;
    return CCD_OK;
}

void ccd_png_destroy(ccd_png* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    void* const device_bufs[] = {p->d_scan, p->d_codes, p->d_blk_bits, p->d_row_adler, p->d_meta, p->d_prev, p->d_lz,
                                 p->d_lz_codes, p->d_lz_flag, p->d_jobs[0], p->d_jobs[1]};
    void* const pinned_bufs[] = {p->h_meta, p->h_jobs[0], p->h_jobs[1]};
    for (void* b : device_bufs) if (b) (void)hipFree(b);
    for (void* b : pinned_bufs) if (b) (void)hipHostFree(b);
    for (hipEvent_t e : p->ev) if (e) (void)hipEventDestroy(e);
    delete p;
}

int ccd_png_set_level(ccd_png* p, int level) {
    if (!p || (level != CCD_PNG_LITERAL && level != CCD_PNG_LZ77)) return CCD_ERR_ARG;
    p->level = level;
    return CCD_OK;
}

int ccd_png_pack_batch(ccd_png* p, const ccd_png_item* items, int n, void* stream) {
    if (!p || !items || n <= 0) return CCD_ERR_ARG;
    PackSize sz;
    if (!validate_and_size(items, n, &sz)) return CCD_ERR_ARG;
    if (hipSetDevice(p->device) != hipSuccess) return CCD_ERR_HIP;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool lz = p->level == CCD_PNG_LZ77;
    int rc = ensure_workspace(p, n, sz, lz, st);
    if (rc != CCD_OK) return rc;
    const int jk = p->flip;
    p->flip ^= 1;
    // this copy of the table was last read two packs ago: normally long finished
    if (p->ev_used[jk] && hipEventSynchronize(p->ev[jk]) != hipSuccess) return CCD_ERR_HIP;
    PngJob* jobs = p->h_jobs[jk];
    fill_jobs(p, jobs, items, n, lz);
    if (hipMemcpyAsync(p->d_jobs[jk], jobs, static_cast<size_t>(n) * sizeof(PngJob), hipMemcpyHostToDevice, st) != hipSuccess)
        rc = CCD_ERR_HIP;
    for (int first = 0; first < n && rc == CCD_OK; first += kMaxBatch)
        rc = launch_set(p, jobs + first, p->d_jobs[jk] + first, std::min(kMaxBatch, n - first), lz, st);
    if (hipEventRecord(p->ev[jk], st) != hipSuccess) rc = CCD_ERR_HIP;
    p->ev_used[jk] = true;
    if (rc != CCD_OK) return rc;
    if (hipMemcpyAsync(p->h_meta, p->d_meta, static_cast<size_t>(n) * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess)
        return CCD_ERR_HIP;
    p->pending = n;
    p->pack_stream = st;
    return CCD_OK;
}

int ccd_png_finish_batch(ccd_png* p, void* stream, int64_t* sizes, int n) {
    if (!p || !sizes || p->pending <= 0 || n != p->pending) return CCD_ERR_ARG;
    if (hipSetDevice(p->device) != hipSuccess) return CCD_ERR_HIP;
    if (hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) return CCD_ERR_HIP;
    // the sizes are behind the pack on the stream the pack was given, whichever stream this call names
    if (p->pack_stream != static_cast<hipStream_t>(stream) && hipStreamSynchronize(p->pack_stream) != hipSuccess) return CCD_ERR_HIP;
    p->pending = 0;
    int rc = CCD_OK;
    for (int i = 0; i < n; ++i) {
        const uint32_t* m = p->h_meta + static_cast<size_t>(i) * 8;
        if (m[4]) { sizes[i] = CCD_ERR_NOMEM; rc = CCD_ERR_NOMEM; }  // the file did not fit `cap` (cannot happen with ccd_png_bound())
        else sizes[i] = static_cast<int64_t>(m[2]);
    }
    return rc;
}

int ccd_png_pack(ccd_png* p, const uint8_t* r, const uint8_t* g, const uint8_t* b, int h, int w, uint8_t* out, size_t cap,
                 void* stream) {
    ccd_png_item it;
    it.r = r; it.g = g; it.b = b; it.h = h; it.w = w; it.out = out; it.cap = cap;
    return ccd_png_pack_batch(p, &it, 1, stream);
}

int64_t ccd_png_finish(ccd_png* p, void* stream) {
    int64_t size = 0;
    const int rc = ccd_png_finish_batch(p, stream, &size, 1);
    return rc < 0 ? rc : size;
}

}  // extern "C"
