// Does a SATISFIED s_waitcnt (nothing outstanding) cost a lone wave an issue slot?  Four independent v_mad_i32_i24 per body, bare,
// with one s_waitcnt lgkmcnt(0) behind them, with one behind each, and - for scale - with one s_nop 0 behind them / behind each.
// (The MLP blocks of the entropy producers carry one s_waitcnt lgkmcnt(n) per weight vector: DESIGN.md 7.)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define REP8(x) x x x x x x x x
#define REP64(x) REP8(REP8(x))
#define PROBE(name, body)                                                               \
    __global__ __launch_bounds__(512) void name(uint64_t* out, uint32_t seed) {         \
        uint32_t v = threadIdx.x + seed, w = v * 3 + 1;                                  \
        uint64_t t0 = __builtin_amdgcn_s_memtime();                                      \
        for (int it = 0; it < 16; ++it)                                                  \
            asm volatile(REP64(body) : "+v"(v), "+v"(w) : : "v10", "v12", "v14", "v16"); \
        uint64_t t1 = __builtin_amdgcn_s_memtime();                                      \
        if ((threadIdx.x & 63) == 0) { out[threadIdx.x / 64] = t1 - t0; out[16] = v + w; } \
    }
#define M(r) "v_mad_i32_i24 " r ", %0, %1, " r "\n"
#define W "s_waitcnt lgkmcnt(0)\n"
#define N "s_nop 0\n"
PROBE(p_bare, M("v10") M("v12") M("v14") M("v16"))
PROBE(p_wait1, M("v10") M("v12") M("v14") M("v16") W)
PROBE(p_wait4, M("v10") W M("v12") W M("v14") W M("v16") W)
PROBE(p_nop1, M("v10") M("v12") M("v14") M("v16") N)
PROBE(p_nop4, M("v10") N M("v12") N M("v14") N M("v16") N)
typedef void (*kern_t)(uint64_t*, uint32_t);
int main() {
    uint64_t* d;
    if (hipMalloc(&d, 256) != hipSuccess) return 1;
    struct { const char* n; kern_t k; } P[] = {{"4 mad", p_bare}, {"4 mad + 1 satisfied s_waitcnt", p_wait1}, {"4 x (mad + satisfied s_waitcnt)", p_wait4},
                                               {"4 mad + 1 s_nop", p_nop1}, {"4 x (mad + s_nop)", p_nop4}};
    for (int threads : {64, 512})
        for (auto& p : P) {
            uint64_t h[8];
            for (int r = 0; r < 2; ++r) { hipLaunchKernelGGL(p.k, dim3(1), dim3(threads), 0, 0, d, 5u); if (hipDeviceSynchronize() != hipSuccess) return 1; }
            if (hipMemcpy(h, d, 64, hipMemcpyDeviceToHost) != hipSuccess) return 1;
            printf("%4d threads  %-34s %8.2f ticks per body of 4 mad (wave 0)\n", threads, p.n, h[0] / (16.0 * 64));
        }
    return 0;
}
