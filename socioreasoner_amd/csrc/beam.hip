// Deterministic beam search on the device (the reference's num_beams > 1: HF GenerationMixin._beam_search with do_sample=False,
// early_stopping=False).  A batch is G groups (prompts) x W beams = B decode rows, group g owning rows g*W .. g*W+W-1.  Three launches per
// decode step, all inside the captured step:
//   k_beam_rowstats  grid (NB, B): every row's logits in chunks of RS_CH floats -> per chunk (max, sum exp(x - max)) and its top-K logits;
//   k_beam_select    one block per group: logZ of each beam (fixed-order merge of the chunk partials), the group's top-K candidates
//                    running[beam] + logit - logZ over the union of its beams' chunk lists, the next running beams, the finished list, the
//                    early-stop flag, the parent / token trace, the new row -> KV-slot map and the copy list of the KV reorder;
//   k_kv_suffix      positions [L0, L1) of every copy-list entry's source slot -> its destination slot, all layers, both caches.
// A row's top-K by logit is its top-K by log-prob, so the group's top-K lies in the union of its beams' lists.  Every reduction runs in a
// fixed order: a group's result does not depend on the other groups of the batch.
#include "kernels.h"
#include "rowstats.h"

namespace {

__global__ __launch_bounds__(RS_T) void k_beam_rowstats(BeamArgs a) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int chunk = blockIdx.x, row = blockIdx.y, NB = gridDim.x;
    rowstats_chunk(a.logits + (size_t)row * a.V, a.V, chunk, a.K, a.part + ((size_t)row * NB + chunk) * (a.K + 1), sv, si);
}

constexpr int SEL_T = 256;

__global__ __launch_bounds__(SEL_T) void k_beam_select(BeamArgs a) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float s_logz[BEAM_MAXW], s_run[BEAM_MAXW];
    __shared__ float c_score[BEAM_MAXK];
    __shared__ int c_flat[BEAM_MAXK];
    __shared__ int s_step;
    const int g = blockIdx.x, tid = threadIdx.x, W = a.W, K = a.K, NB = a.NB;
    const int r0 = g * W;
    if (tid == 0) s_step = a.step_ctr ? a.step_ctr[r0] : a.step;
    __syncthreads();
    const int t = s_step;
    BeamTrace* tr = a.trace + (size_t)t * a.trace_ld + r0;
    if (a.done[g]) {                            // a stopped group freezes: no new entries, no copies; its rows feed pad
        if (tid < W) {
            tr[tid] = BeamTrace{-1, a.pad_id};
            a.next_tok[r0 + tid] = a.pad_id;
            if (a.copies) a.copies[r0 + tid] = make_int4(-1, -1, 0, 0);
        }
        return;
    }
    // logZ of every beam: the chunk partials merged in chunk order
    if (tid < W) {
        const BeamPart* p = a.part + (size_t)(r0 + tid) * NB * (K + 1);
        float M = -INFINITY;
        for (int c = 0; c < NB; ++c) M = fmaxf(M, p[(size_t)c * (K + 1)].v);
        float S = 0.f;
        for (int c = 0; c < NB; ++c) S += __int_as_float(p[(size_t)c * (K + 1)].i) * expf(p[(size_t)c * (K + 1)].v - M);
        s_logz[tid] = M + logf(S);
        s_run[tid] = a.scores[r0 + tid];
    }
    __syncthreads();
    // the group's top-K over W x NB x K candidates (score desc, flat index beam * V + token asc), same scheme as the chunk top-K
    const int per_row = NB * K, n_cand = W * per_row;
    auto cand = [&](int c, float& sc, int& fl) {
        const int b = c / per_row, q = c - b * per_row;
        const BeamPart e = a.part[(size_t)(r0 + b) * NB * (K + 1) + (size_t)(q / K) * (K + 1) + 1 + q % K];
        if (e.i == 0x7fffffff) { sc = -INFINITY; fl = 0x7fffffff; return; }
        sc = s_run[b] + (e.v - s_logz[b]);
        fl = b * a.V + e.i;
    };
    auto own_best = [&](float tv, int ti, float& bv, int& bi) {
        bv = -INFINITY; bi = 0x7fffffff;
        for (int c = tid; c < n_cand; c += SEL_T) {
            float sc; int fl;
            cand(c, sc, fl);
            if (fl != 0x7fffffff && better(tv, ti, sc, fl) && better(sc, fl, bv, bi)) { bv = sc; bi = fl; }
        }
    };
    float bv; int bi;
    own_best(INFINITY, -1, bv, bi);
    for (int r = 0; r < K; ++r) {
        float wv = bv; int wi = bi;
        block_best(wv, wi, sv, si);
        if (tid == 0) { c_score[r] = wv; c_flat[r] = wi; }
        if (wi == bi && wi != 0x7fffffff) own_best(wv, wi, bv, bi);
    }
    __syncthreads();
    if (tid != 0) return;
    // ---- serial part (K <= 64 candidates, W <= 8 beams)
    const bool last = t + 1 >= a.max_new;
    const float denom = (float)pow((double)(t + 1), (double)a.lp);
    bool hit[BEAM_MAXK];
    float rs[BEAM_MAXK];
    for (int k = 0; k < K; ++k) {
        const int tok = c_flat[k] % a.V;
        bool h = last;
        for (int q = 0; q < a.n_eos; ++q) h |= tok == a.eos[q];
        hit[k] = h;
        rs[k] = c_score[k] + (h ? -1.0e9f : 0.0f);
    }
    // next running beams: the top W of rs (index asc on ties)
    int sel[BEAM_MAXW];
    bool used[BEAM_MAXK];
    for (int k = 0; k < K; ++k) used[k] = false;
    for (int j = 0; j < W; ++j) {
        int best = -1;
        for (int k = 0; k < K; ++k) if (!used[k] && (best < 0 || rs[k] > rs[best])) best = k;
        used[best] = true;
        sel[j] = best;
    }
    // finished list: the first W candidates that hit, scored cum / len^lp, merged (old entries first) into the best W
    BeamFin* fin = a.fin + r0;
    int nf = a.fin_n[g];
    for (int k = 0; k < W; ++k) {
        if (!hit[k]) continue;
        const BeamFin nw{c_score[k] / denom, t, c_flat[k] / a.V, c_flat[k] % a.V};
        int at = nf;                                   // first position with a strictly lower score: equal scores keep the older entry first
        for (int q = 0; q < nf; ++q) if (nw.score > fin[q].score) { at = q; break; }
        if (at >= W) continue;
        for (int q = (nf < W ? nf : W - 1); q > at; --q) fin[q] = fin[q - 1];
        fin[at] = nw;
        if (nf < W) ++nf;
    }
    a.fin_n[g] = nf;
    // parents, tokens, scores; the KV reorder: the first child of a parent inherits its slot, the other children take the slots of the
    // parents without children and get a copy of the parent's generated suffix [prompt_len, ctx)
    int par[BEAM_MAXW], slot_old[BEAM_MAXW], slot_new[BEAM_MAXW];
    bool claimed[BEAM_MAXW];
    for (int j = 0; j < W; ++j) { claimed[j] = false; slot_old[j] = a.slots ? a.slots[r0 + j] : 0; }
    for (int j = 0; j < W; ++j) {
        const int k = sel[j];
        par[j] = c_flat[k] / a.V;
        const int tok = c_flat[k] % a.V;
        a.scores[r0 + j] = rs[k];
        a.next_tok[r0 + j] = tok;
        tr[j] = BeamTrace{par[j], tok};
        slot_new[j] = -1;
        if (!claimed[par[j]]) { claimed[par[j]] = true; slot_new[j] = slot_old[par[j]]; }
    }
    if (a.slots) {
        const int ctx = a.ctx_len[r0], L0 = a.prompt_len[g];
        int f = 0, nc = 0;
        for (int j = 0; j < W; ++j) {
            if (slot_new[j] >= 0) continue;
            while (claimed[f]) ++f;
            claimed[f] = true;
            slot_new[j] = slot_old[f];
            a.copies[r0 + nc++] = make_int4(slot_old[par[j]], slot_new[j], L0, ctx);
        }
        for (int q = nc; q < W; ++q) a.copies[r0 + q] = make_int4(-1, -1, 0, 0);
        for (int j = 0; j < W; ++j) a.slots[r0 + j] = slot_new[j];
    }
    // early stop (HF's heuristic for early_stopping=False): a full finished list that the best running beam cannot beat
    if (nf == W && rs[sel[0]] / denom <= fin[W - 1].score) { a.done[g] = 1; a.stop_step[g] = t; }
}

// positions [L0, L1) of slot src -> slot dst for every copy-list entry; grid (NX, layer x kvh), each block strides over the entries' chunks.
// kcache: 16 chunks of 16 B per position; vtcache: 128 rows, chunks aligned to 8 positions, partial at both ends (the load reads the whole
// aligned 16 B -- in bounds, max_ctx % 64 == 0 -- the stores write only [L0, L1))
constexpr int KS_T = 256;

__global__ __launch_bounds__(KS_T) void k_kv_suffix(KvSuffixArgs a) {
    const int layer = blockIdx.y / a.n_kvh, h = blockIdx.y - layer * a.n_kvh;
    const size_t head = (size_t)a.max_ctx * 128;
    const size_t slot_elems = head * a.n_kvh;
    const size_t base = (size_t)layer * (size_t)a.layer_stride + (size_t)h * head;
    const int stride = gridDim.x * KS_T;
    for (int n = 0; n < a.n; ++n) {
        const int4 e = a.copies[n];
        const int src = e.x, dst = e.y, L0 = e.z, L1 = e.w;
        if (src < 0 || L1 <= L0) continue;
        const int nK = (L1 - L0) * 16, q0 = L0 >> 3, cpr = ((L1 - 1) >> 3) - q0 + 1, nV = 128 * cpr;
        for (int c = blockIdx.x * KS_T + threadIdx.x; c < nK + nV; c += stride) {
            if (c < nK) {
                const size_t off = (size_t)L0 * 128 + (size_t)c * 8;
                *reinterpret_cast<uint4*>(a.kcache + base + (size_t)dst * slot_elems + off) =
                    *reinterpret_cast<const uint4*>(a.kcache + base + (size_t)src * slot_elems + off);
            } else {
                const int v = c - nK, r = v / cpr, q = q0 + (v - r * cpr);
                const size_t off = (size_t)r * a.max_ctx + (size_t)q * 8;
                const uint4 x = *reinterpret_cast<const uint4*>(a.vtcache + base + (size_t)src * slot_elems + off);
                const int lo = max(L0 - q * 8, 0), hi = min(L1 - q * 8, 8);
                bf16_t* p = a.vtcache + base + (size_t)dst * slot_elems + off;
                if (lo == 0 && hi == 8) *reinterpret_cast<uint4*>(p) = x;
                else {
                    const bf16_t* xs = reinterpret_cast<const bf16_t*>(&x);
                    for (int k = lo; k < hi; ++k) p[k] = xs[k];
                }
            }
        }
    }
}

}  // namespace

int launch_beam_rowstats(hipStream_t s, const BeamArgs& a) {
    if (a.K < 1 || a.K > BEAM_MAXK || a.NB != beam_nb(a.V) || a.G * a.W < 1) return -22;
    hipLaunchKernelGGL(k_beam_rowstats, dim3(a.NB, a.G * a.W), dim3(RS_T), 0, s, a);
    SR_CHECK_LAUNCH();
    return 0;
}

int launch_beam_select(hipStream_t s, const BeamArgs& a) {
    if (a.K < 1 || a.K > BEAM_MAXK || a.W < 1 || a.W > BEAM_MAXW || a.G < 1 || a.K < a.W) return -22;
    hipLaunchKernelGGL(k_beam_select, dim3(a.G), dim3(SEL_T), 0, s, a);
    SR_CHECK_LAUNCH();
    return 0;
}

int launch_kv_suffix(hipStream_t s, const KvSuffixArgs& a) {
    if (a.n <= 0) return 0;
    if (a.max_ctx % 64 || a.n_layers < 1 || a.n_kvh < 1 || a.nx < 1) return -22;
    hipLaunchKernelGGL(k_kv_suffix, dim3(a.nx, a.n_layers * a.n_kvh), dim3(KS_T), 0, s, a);
    SR_CHECK_LAUNCH();
    return 0;
}
