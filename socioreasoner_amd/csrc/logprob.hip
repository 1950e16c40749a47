// Log-probs of generated tokens (sr_logprobs; vLLM's logprobs=N with raw_logprobs): for the float32 logits row x that produced a token,
// lp = x[tok] - logsumexp(x) and the row's top-N logits as (id, x[id] - logsumexp(x)).  Two launches at the tail of the captured step:
//   k_lp_parts   grid (NB, records): the beam search's chunk pass (rowstats.h) -> per chunk (max, sum exp(x - max)) and its top-K;
//   k_lp_finish  one wave per record: logsumexp merged in chunk order (a lane per chunk, the sum in a fixed order), the top-N over the
//                chunk lists, the token (given, or the arg-max under k_step's rule: lowest id among the maxima), the record.
// Every reduction runs in a fixed order and reads one logits row: a record does not depend on the batch, the row index or the launch form.
#include "kernels.h"
#include "rowstats.h"

namespace {

// a record that is not due (engine log only): the row has finished or its log is full
__device__ __forceinline__ bool lp_due(const LogprobArgs& a, int rec) { return !a.step || (!a.finished[rec] && a.step[rec] < a.max_new); }

__global__ __launch_bounds__(RS_T) void k_lp_parts(LogprobArgs a) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int chunk = blockIdx.x, rec = blockIdx.y, NB = gridDim.x;
    if (!lp_due(a, rec)) return;
    const int row = a.row_map ? a.row_map[rec] : rec;
    rowstats_chunk(a.logits + (size_t)row * a.ld, a.V, chunk, max(a.top_n, 1), a.part + ((size_t)rec * NB + chunk) * LP_PW, sv, si);
}

__global__ __launch_bounds__(64) void k_lp_finish(LogprobArgs a, int NB) {
    const int rec = blockIdx.x, lane = threadIdx.x;
    if (!lp_due(a, rec)) return;
    const size_t dst = a.step ? (size_t)rec * a.max_new + a.step[rec] : (size_t)rec;
    const BeamPart* p = a.part + (size_t)rec * NB * LP_PW;
    // logsumexp: lane c takes chunk c's partial (one load and one expf per lane instead of a serial walk), the maximum over the wave, then the
    // terms added in chunk order -- every lane adds the same sequence, so all hold the same sum
    float M = -INFINITY;
    for (int c = lane; c < NB; c += 64) M = fmaxf(M, p[(size_t)c * LP_PW].v);
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    float S = 0.f;
    for (int c0 = 0; c0 < NB; c0 += 64) {
        float t = 0.f;
        if (c0 + lane < NB) {
            const BeamPart e = p[(size_t)(c0 + lane) * LP_PW];
            if (e.v != -INFINITY) t = __int_as_float(e.i) * expf(e.v - M);
        }
        const int n = min(64, NB - c0);
        for (int k = 0; k < n; ++k) S += __shfl(t, k, 64);
    }
    const float lse = M + logf(S);
    // top-K over the NB x K chunk entries (logit desc, token asc): K rounds, each the best entry strictly below the previous winner
    const int K = max(a.top_n, 1), n_cand = NB * K;
    float wv[LP_MAXN]; int wi[LP_MAXN];
    float tv = INFINITY; int ti = -1;
#pragma unroll
    for (int r = 0; r < LP_MAXN; ++r) {
        wv[r] = 0.f; wi[r] = -1;
        if (r >= K) continue;
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int c = lane; c < n_cand; c += 64) {
            const BeamPart e = p[(size_t)(c / K) * LP_PW + 1 + c % K];
            if (e.i != 0x7fffffff && better(tv, ti, e.v, e.i) && better(e.v, e.i, bv, bi)) { bv = e.v; bi = e.i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        wv[r] = bv; wi[r] = bi; tv = bv; ti = bi;
    }
    if (lane != 0) return;
    const int row = a.row_map ? a.row_map[rec] : rec;
    int tok = wi[0];
    float xt = wv[0];
    if (a.chosen) {
        tok = (int)a.chosen[rec];
        xt = (tok >= 0 && tok < a.V) ? a.logits[(size_t)row * a.ld + tok] : lse;      // (a token outside the vocabulary cannot be looked up: lp 0)
    }
    a.lp[dst] = xt - lse;
    if (a.tok_out) a.tok_out[dst] = tok;
    if (a.top_ids) {
#pragma unroll
        for (int r = 0; r < LP_MAXN; ++r) {
            const bool on = r < a.top_n && wi[r] != 0x7fffffff;
            a.top_ids[dst * LP_MAXN + r] = on ? wi[r] : -1;
            a.top_lp[dst * LP_MAXN + r] = on ? wv[r] - lse : 0.f;
        }
    }
}

__device__ __forceinline__ void lp_clear(float* lp, int* top_ids, float* top_lp, size_t rec) {
    lp[rec] = 0.f;
    for (int r = 0; r < LP_MAXN; ++r) { top_ids[rec * LP_MAXN + r] = -1; top_lp[rec * LP_MAXN + r] = 0.f; }
}

__global__ __launch_bounds__(256) void k_lp_clear(int n_rec, float* lp, int* top_ids, float* top_lp) {
    const int rec = blockIdx.x * 256 + threadIdx.x;
    if (rec < n_rec) lp_clear(lp, top_ids, top_lp, rec);
}

// one block per admitted sequence
__global__ __launch_bounds__(256) void k_lp_admit(LogprobAdmitArgs a) {
    const int i = blockIdx.x;
    const size_t base = (size_t)a.rows[i] * a.max_new;
    for (int t = threadIdx.x; t < a.max_new; t += 256) {
        lp_clear(a.lp, a.top_ids, a.top_lp, base + t);
        if (t == 0 && a.src_lp) {
            a.lp[base] = a.src_lp[i];
            for (int r = 0; r < LP_MAXN; ++r) { a.top_ids[base * LP_MAXN + r] = a.src_ids[i * LP_MAXN + r]; a.top_lp[base * LP_MAXN + r] = a.src_tlp[i * LP_MAXN + r]; }
        }
    }
}

}  // namespace

int launch_logprobs(hipStream_t s, const LogprobArgs& a) {
    if (a.n < 1 || a.V < 1 || a.ld < a.V || a.top_n < 0 || a.top_n > LP_MAXN || !a.logits || !a.part || !a.lp || (a.top_ids == nullptr) != (a.top_lp == nullptr) ||
        (a.step && (!a.finished || a.max_new < 1)))
        return -22;
    const int NB = beam_nb(a.V);
    hipLaunchKernelGGL(k_lp_parts, dim3(NB, a.n), dim3(RS_T), 0, s, a);
    SR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lp_finish, dim3(a.n), dim3(64), 0, s, a, NB);
    SR_CHECK_LAUNCH();
    return 0;
}

int launch_logprob_admit(hipStream_t s, const LogprobAdmitArgs& a) {
    if (a.n < 1 || a.max_new < 1) return -22;
    hipLaunchKernelGGL(k_lp_admit, dim3(a.n), dim3(256), 0, s, a);
    SR_CHECK_LAUNCH();
    return 0;
}

int launch_logprob_clear(hipStream_t s, int n_rec, float* lp, int* top_ids, float* top_lp) {
    if (n_rec < 1) return 0;
    hipLaunchKernelGGL(k_lp_clear, dim3((n_rec + 255) / 256), dim3(256), 0, s, n_rec, lp, top_ids, top_lp);
    SR_CHECK_LAUNCH();
    return 0;
}
