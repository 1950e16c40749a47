// Row statistics over float32 logits in chunks of RS_CH (beam.hip, logprob.hip): the 256-thread block reductions (fixed order, every thread
// receives the result) and the chunk pass itself.
#pragma once
#include "kernels.h"

constexpr int RS_T = 256;

__device__ __forceinline__ bool better(float v1, int i1, float v2, int i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }

// block-wide arg-best of (v, i) over 256 threads (value desc, index asc); every thread receives the winner.  `sv` / `si`: 4 floats / ints
// of LDS, reused by consecutive calls (the trailing barrier keeps a later call from overwriting what this one still reads)
__device__ __forceinline__ void block_best(float& v, int& i, float* sv, int* si) {
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sv[w] = v; si[w] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
    for (int k = 1; k < RS_T / 64; ++k) if (better(sv[k], si[k], v, i)) { v = sv[k]; i = si[k]; }
    __syncthreads();
}

__device__ __forceinline__ float block_sum(float x, float* sv) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sv[w] = x;
    __syncthreads();
    const float r = (sv[0] + sv[1]) + (sv[2] + sv[3]);
    __syncthreads();
    return r;
}

constexpr int RS_PER = RS_CH / RS_T;     // logits per thread of a chunk

// One chunk of one logits row `x` (V entries), by one 256-thread block: out[0] = (chunk max, bits of sum exp(x - max)), out[1 .. K] = the
// chunk's top-K (logit, token) by (logit desc, token asc); entries past the chunk's end are (-inf, 0x7fffffff).  Reads nothing at or past x[V]
__device__ __forceinline__ void rowstats_chunk(const float* x, int V, int chunk, int K, BeamPart* out, float* sv, int* si) {
    const int tid = threadIdx.x;
    const int c0 = chunk * RS_CH;
    float v[RS_PER];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < RS_PER; ++k) {
        const int t = c0 + k * RS_T + tid;
        v[k] = t < V ? x[t] : -INFINITY;
        m = fmaxf(m, v[k]);
    }
    int dummy = 0;
    block_best(m, dummy, sv, si);          // (max only: the index is irrelevant)
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < RS_PER; ++k) s += v[k] == -INFINITY ? 0.f : expf(v[k] - m);
    s = block_sum(s, sv);
    if (tid == 0) out[0] = BeamPart{m, __float_as_int(s)};
    // top-K of the chunk: K rounds of a block arg-best over the threads' own best entries strictly below the previous winner (the winners
    // fall in the total order, so a thread's next candidate is its best entry below the last one taken; only the winning thread rescans)
    auto own_best = [&](float tv, int ti, float& bv, int& bi) {
        bv = -INFINITY; bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < RS_PER; ++k) {
            const int t = c0 + k * RS_T + tid;
            if (t < V && better(tv, ti, v[k], t) && better(v[k], t, bv, bi)) { bv = v[k]; bi = t; }
        }
    };
    float bv; int bi;
    own_best(INFINITY, -1, bv, bi);
    for (int r = 0; r < K; ++r) {
        float wv = bv; int wi = bi;
        block_best(wv, wi, sv, si);
        if (tid == 0) out[1 + r] = BeamPart{wv, wi};
        if (wi == bi && wi != 0x7fffffff) own_best(wv, wi, bv, bi);
    }
}
