// libsocior engine: the C ABI of include/socior.h and the host-side orchestration of the hot path
// (ViT -> merger -> LM prefill -> greedy decode), one engine per GPU/process.
//
// What it replaces in the reference (paths relative to /root/reference): the engine behind
// VllmStrategy.generate (roll/distributed/strategy/vllm_strategy.py:114-141), i.e. vLLM's Qwen2.5-VL executor; the
// arithmetic follows HF's eager implementation (`hf:` = transformers/models/qwen2_5_vl/modeling_qwen2_5_vl.py) which
// is the reference's CPU/eager path (roll/distributed/strategy/hf_strategy.py:49-94).
//
// Memory: one caller-provided workspace carved by a bump allocator: weights (engine layout), activations sized by the
// capacities in sr_config, KV cache (K [layer][slot][kvh][ctx][128], V^T [layer][slot][kvh][128][ctx]), control arrays.
// Decode runs from device-resident state (ctx_len, positions, current token, step) so that ONE captured hipGraph
// replays for every step (launch-bound inner loop -> graph, per the MI355X guide).
#include "../../include/socior.h"
#include "kernels.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace {

thread_local char g_err[512] = "ok";

constexpr int MAXB = 128;     // batch rows an engine can be configured with (the reference's request-level mode keeps up to 128 requests
                              // in flight per worker: /root/reference/roll/distributed/scheduler/generate_scheduler.py:57)
constexpr int SPLITK_KS = 4, SPLITK_ROWS = 1024;      // split-K of the residual GEMMs of small prefills (prefill_splitk below)
struct VitBlockW {
    bf16_t *norm1, *qkv_w, *qkv_b, *proj_w, *proj_b, *norm2, *gu_w, *gu_b, *down_w, *down_b;
    // v_weight_dtype = 2: fp8 images (tiled8) + per-output-channel scales of the four linears, quantised FROM the bf16 masters above (which stay)
    unsigned char *qkv_w8 = nullptr, *proj_w8 = nullptr, *gu_w8 = nullptr, *down_w8 = nullptr;
    float *qkv_s = nullptr, *proj_s = nullptr, *gu_s = nullptr, *down_s = nullptr;
    unsigned char dirty[4] = {0, 0, 0, 0};      // a tensor of the matrix was (re)loaded since its last quantisation
};
struct LmLayerW {
    bf16_t *ln1, *qkv_w, *qkv_b, *o_w, *ln2, *gu_w, *down_w;
    // lm_weight_dtype = 1: fp8 images (tiled8) + per-output-channel scales of the four linears (null in bf16 mode)
    unsigned char *qkv_w8 = nullptr, *o_w8 = nullptr, *gu_w8 = nullptr, *down_w8 = nullptr;
    float *qkv_s = nullptr, *o_s = nullptr, *gu_s = nullptr, *down_s = nullptr;
    // HF tensors (re)loaded into each fused matrix since its last quantisation: qkv {q,k,v} = 7, o = 1, gate/up = 3, down = 1
    unsigned char dirty[4] = {0, 0, 0, 0};
};

struct Arena {
    char* base = nullptr;
    size_t off = 0, cap = 0;
    template <class T>
    T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

inline int rup(int a, int b) { return (a + b - 1) / b * b; }

uint32_t fnv1a32(const char* s) {
    uint32_t h = 2166136261u;
    for (; *s; ++s) { h ^= (unsigned char)*s; h *= 16777619u; }
    return h;
}
uint32_t mix32h(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
bf16_t host_f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}

}  // namespace

// ---- SR_* switches: the environment is read here and nowhere else in the library
static SrSwitches g_sw;
static bool g_sw_loaded = false;
static int env_int(const char* name, int dflt) { const char* v = getenv(name); return (v && *v) ? atoi(v) : dflt; }
static void load_switches() {
    g_sw.splitk = env_int("SR_SPLITK", 0);
    g_sw.gemm_bm = env_int("SR_GEMM_BM", 0);
    g_sw.gemm_ring = env_int("SR_GEMM_RING", 1);
    g_sw.gemm256 = env_int("SR_GEMM256", 1);
    g_sw.fuse_qkv = env_int("SR_FUSE_QKV", 1);
    g_sw.g256_group = env_int("SR_G256_GROUP", 4);
    if (g_sw.g256_group < 1) g_sw.g256_group = 4;
    g_sw.attn2 = env_int("SR_ATTN2", 1);
    g_sw.attn_win64 = env_int("SR_ATTN_WIN64", 1);
    g_sw.attn_vasm = env_int("SR_ATTN_VASM", 1);
    g_sw.sam_f32_split = env_int("SR_SAM_F32_SPLIT", 1);
    g_sw.gemv_counted = env_int("SR_GEMV_COUNTED", 1);
    g_sw.gemv_xlds = env_int("SR_GEMV_XLDS", 11);
    g_sw_loaded = true;
}
const SrSwitches& sr_switches() {
    if (!g_sw_loaded) load_switches();
    return g_sw;
}

// The captured forms of one decode step (the slots of sr_engine::graphs)
enum StepKind {
    STEP_GREEDY,            // sr_decode, sr_rows_step: k_step reduces the LM head's arg-max partials
    STEP_CALLER_GREEDY,     // sr_decode_step feeding the engine's greedy token
    STEP_CALLER_CHOSEN,     // sr_decode_step feeding the caller's token (d_chosen)
    STEP_SAMPLED,           // sr_decode_sample: bookkeeping + forward + k_sample
    STEP_BEAM,              // sr_decode_beam: bookkeeping + forward + row statistics + select + KV suffix copies
    STEP_ROWS_SAMPLED,      // sr_rows_step under sr_rows_sampling
    STEP_ROWS_PERROW,       // sr_rows_step under sr_rows_per_row
    STEP_KINDS
};
// everything a captured step bakes in BY VALUE (step_key fills it from the step's description); compared as a whole with memcmp
struct StepKey {
    int B, n_eos, pad_id;
    int top_k; float inv_temp, top_p, rep_penalty; unsigned seed;      // the sampled kinds
    int W, K, max_new; float length_penalty;                           // beam
    int lp;                                                            // token log-probs (sr_logprobs): top_n + 1 when the step records them, 0 = off
};
static_assert(sizeof(StepKey) == 13 * 4, "no padding");
struct StepGraph { hipGraphExec_t exec = nullptr; StepKey key{}; };

struct sr_engine {
    sr_config c;
    // derived geometry
    int v_hd, v_pd, v_pd_pad, v_inter_pad, v_mh, t_inter_pad, t_qn, t_group;
    int ks_down;                 // cross-block split-K (float32 slabs) of the decode down-projection
    Arena ar;
    size_t weights_begin = 0, weights_end = 0;
    // ---- weights
    bf16_t* patch_w;
    std::vector<VitBlockW> vb;
    bf16_t *ln_q, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
    unsigned char *fc1_w8 = nullptr, *fc2_w8 = nullptr; float *fc1_s = nullptr, *fc2_s = nullptr; unsigned char fc_dirty[2] = {0, 0};   // v_weight_dtype 2 (as VitBlockW)
    bf16_t *embed, *final_norm;
    std::vector<LmLayerW> ll;
    bf16_t* lut;       // [3*256] normalise LUT
    float* inv_freq;   // [64]
    bf16_t *rope_cos, *rope_sin;   // [max_ctx + 1][64]
    // ---- ViT activations
    bf16_t *v_pix, *v_x, *v_xn, *v_qkv, *v_attn, *v_act, *v_vt, *v_m1;
    int v_vt_stride;
    bool v_paired = false;       // ViT q / k channels stored in the paired order (head_dim / 2 % 8 == 0): see vit_qk_perm
    float *v_cos, *v_sin;
    int *v_rowmap_embed, *v_rowmap_merge;
    // v_weight_dtype 2: MX-quantised GEMM input of the tower's linears (elements + e8m0 scales [K/128][v_rows_pad][4]); the tower's own, so a
    // ViT pass on one stream never meets a prefill's t_q8 / t_qs on another
    unsigned char *v_q8 = nullptr, *v_qs = nullptr; int v_rows_pad = 0; size_t v_qs_bytes = 0;
    AttnWork *v_work_win, *v_work_full, *v_work_full128;     // full attention: 64-query items (k_attn_prefill) and 128-query items (k_attn_prefill2)
    int v_nwork_full128; bool v_full_aligned;
    bool v_win_all64;              // every window of the cached grids is a full 8 x 8 merge-unit window (64 tokens): k_attn_win64 applies
    int v_nwork_win = 0, v_nwork_full = 0;
    std::vector<int64_t> v_grid_cached;
    // ---- LM activations
    bf16_t *t_x, *t_xn, *t_qkv, *t_attn, *t_act;
    float* t_slabs = nullptr;    // [SPLITK_KS][SPLITK_ROWS][hidden] float32: split-K partial products of the residual GEMMs of a SMALL prefill
    int n_slots = 0;                         // KV-cache slots (>= max_batch): spare slots take admissions prefilled UNDER the running rows' decode
    int staged_n = 0, staged_off = 0;        // sequences of a staged admission that still wait for rows / already installed
    bf16_t *d_xadm = nullptr, *d_xadm_n = nullptr; int* d_adm_slots = nullptr; int h_rows[MAXB];
    unsigned char *t_q8 = nullptr, *t_qs = nullptr; int t_rows_pad = 0;     // lm_weight_dtype 2: MX-quantised GEMM input of the prefill
    int *t_src, *t_pos3, *t_slot, *t_idx, *t_lastrow;
    AttnWork* t_work;
    // ---- decode state (device)
    bf16_t *d_xa, *d_xb, *d_xn, *d_qkv, *d_attn, *d_act, *d_scores;    // d_xa / d_xb: residual stream ping-pong
    float *d_logits, *d_slabs, *d_amax_val;
    float* d_row_cs = nullptr;               // [MAXB][128] rotary cos | sin of every row's current position (k_step -> decode attention)
    unsigned* d_px = nullptr;                // [256] x-stationary GEMVs: 8 ticket shards + done count (k_gemv_px; zero between launches), word 160 = CU limit (sr_rows_set_cus)
    int *d_amax_idx, *d_cur_tok, *d_ctx_len, *d_pos, *d_finished, *d_step, *d_slots, *d_eos, *d_tokens;
    int n_part = 0;      // LM-head blocks = partial argmax entries per row
    // continuous batching (sr_rows_*): admission scratch so that a prefill never touches the pending tokens of running rows
    float *d_logits_adm = nullptr, *d_amax_val_adm = nullptr;
    int *d_amax_idx_adm = nullptr, *d_row_limit = nullptr, *d_ngen = nullptr, *d_adm = nullptr;   // d_adm: [rows | ctx | pos | limit | first_tok] x MAXB
    int* d_fan = nullptr;          // fan-out admission: [prompt of each staged sequence] x MAXB | [src slot | L | first fork index | forks - 1] x MAXB
    bool rows_mode = false;
    bool finalized = false;        // sr_finalize_weights ran (fp8 mode: the LM linears are quantised)
    bf16_t *kcache, *vtcache;
    size_t kv_layer_elems;
    // ---- host staging (pinned) + its device mirror
    char* h_stage = nullptr;
    size_t stage_bytes = 0;
    char* d_stage = nullptr;
    hipEvent_t ev_copy = nullptr;
    bool copy_pending = false;
    // ---- decode graph cache (step_graph): [step kind][px_mode], px_mode = the decode step on the whole chip / on a CU-limited stream
    // (x-stationary GEMVs, sr_rows_set_cus); the continuous batcher alternates between the two, so both forms stay cached
    StepGraph graphs[STEP_KINDS][2];
    int px_mode = 0;
    int device = 0;                     // the GPU the workspace lives on: every C-ABI entry makes it current (per-thread HIP state)
    hipStream_t cap_stream = nullptr;   // used only to CAPTURE the decode step (the caller's stream may be the null stream)
    long long *d_chosen = nullptr, *d_next = nullptr, *d_sampled = nullptr;
    unsigned* d_seen = nullptr;    // [MAXB][seen_words] token bitmask for the repetition penalty
    int seen_words = 0;
    // continuous batching with sampling (sr_rows_sampling): parameters shared by all rows; 0 temperature = greedy
    float rows_temp = 0.f, rows_topp = 1.f; int rows_topk = 0; unsigned rows_seed = 0, adm_count = 0;
    long long* d_adm_pick = nullptr;
    // per-request sampling in the continuous batcher (sr_rows_per_row, sr_admit_sampling / sr_admit_stage_sampling): allocated on first use.
    // rp_rows [MAXB] / rp_stage [MAXB]: the parameter table of the batch rows / of the staged sequences; rp_seen [n_slots][seen_words]: one
    // repetition-penalty bitmap per KV slot; h_rp: pinned upload buffer of the staged entries
    void* rp_mem = nullptr; RowParams *rp_rows = nullptr, *rp_stage = nullptr, *h_rp = nullptr; unsigned* rp_seen = nullptr;
    bool rows_perrow = false;       // sr_rows_step replays the per-row graph
    bool staged_rp = false;         // the staged admission drew its first tokens under its table entries (and marked its slots' bitmaps)
    int prefilled_B = 0;
    int pre_len[MAXB], pre_slot[MAXB], pre_pos[MAXB];   // static prefill: every sequence's length, KV slot and last position (sr_decode_beam)
    // beam search (sr_decode_beam): device state allocated on first use, freed on destroy
    void* beam_mem = nullptr;
    BeamPart* bm_part = nullptr; float* bm_scores = nullptr; long long* bm_tok = nullptr; BeamTrace* bm_trace = nullptr; BeamFin* bm_fin = nullptr;
    int *bm_fin_n = nullptr, *bm_done = nullptr, *bm_stop = nullptr, *bm_eos = nullptr, *bm_plen = nullptr, *bm_fan = nullptr; int4* bm_copies = nullptr;
    // token log-probs (sr_logprobs): allocated on first use, freed on destroy.  lp_n: -1 = off, else the top_n in force.  lp_log / lp_ids /
    // lp_tlp: the log [max_batch][max_new_tokens] (x LP_MAXN); lps_*: the position-0 records of the staged sequences [MAXB]; lp_part /
    // lp_part_adm: chunk partials of the decode step / of an admission (which may run on another stream under the steps)
    void* lp_mem = nullptr; int lp_n = -1;
    float *lp_log = nullptr, *lp_tlp = nullptr, *lps_lp = nullptr, *lps_tlp = nullptr; int *lp_ids = nullptr, *lps_ids = nullptr;
    BeamPart *lp_part = nullptr, *lp_part_adm = nullptr;
    bool staged_lp = false;        // the staged admission recorded its first tokens
    int h_ctx_hi = 0;              // longest context any slot can have reached (prefill length + decode steps issued)
    // ---- bookkeeping
    std::map<std::string, bool> loaded;
    char err[512];
};

namespace {

// HIP's current device is per-thread state (default 0): make the engine's device current at every entry, so that a
// caller on a fresh thread (the request-level server loop) launches, copies and captures on the right GPU
inline void enter(const sr_engine* e) { if (e) (void)hipSetDevice(e->device); }

int fail(sr_engine* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    snprintf(g_err, sizeof g_err, "%s", buf);
    if (e) snprintf(e->err, sizeof e->err, "%s", buf);
    return code;
}
#define SR_TRY(expr)                                                                                          \
    do {                                                                                                      \
        int rc_ = (expr);                                                                                     \
        if (rc_ != 0) return fail(e, rc_, "%s failed with %d (%s) at %s:%d", #expr, rc_,                       \
                                  rc_ > 0 ? hipGetErrorString((hipError_t)rc_) : "invalid argument", __FILE__, __LINE__); \
    } while (0)

const char* validate(const sr_config& c) {
    if (c.v_hidden <= 0 || c.v_heads <= 0 || c.v_hidden % c.v_heads) return "v_hidden/v_heads";
    const int hd = c.v_hidden / c.v_heads;
    if (hd != 80 && hd != 128) return "vision head_dim must be 80 or 128";
    if (c.v_hidden % 64) return "v_hidden must be a multiple of 64";
    if (c.v_merge != 2 || c.v_temporal < 1 || c.v_patch < 1) return "v_merge must be 2";
    if (c.v_out_hidden != c.t_hidden) return "v_out_hidden must equal t_hidden";
    if (c.t_head_dim != 128) return "t_head_dim must be 128";
    if (c.t_hidden % 64 || c.t_vocab % 16) return "t_hidden % 64, t_vocab % 16";
    if (c.t_hidden > 2048) return "t_hidden must be <= 2048 (the decode RMSNorm and fragment-ordered activation kernels are sized for SocioReasoner-3B)";
    if (c.t_heads % c.t_kv_heads || c.t_heads / c.t_kv_heads > 16) return "GQA group must divide and be <= 16";
    if (c.mrope_section[0] + c.mrope_section[1] + c.mrope_section[2] != 64) return "mrope_section must sum to 64";
    if (c.max_batch < 1 || c.max_batch > MAXB) return "max_batch in 1..128";
    if (c.kv_slots != 0 && (c.kv_slots < c.max_batch || c.kv_slots > 2 * MAXB)) return "kv_slots 0 (= max_batch) or max_batch..256";
    if (c.max_ctx < 64 || c.max_ctx % 64) return "max_ctx multiple of 64";
    if (c.lm_weight_dtype < 0 || c.lm_weight_dtype > 2) return "lm_weight_dtype 0 (bf16), 1 (fp8 e4m3 weights, per-channel scale) or 2 (1 + MX fp8 activations in prefill)";
    if (c.lm_weight_dtype == 2 && (c.t_hidden % 256 || ((c.t_heads + 2 * c.t_kv_heads) * 128) % 256 || c.t_hidden / 128 < 2))
        return "lm_weight_dtype 2: the block-scaled fp8 GEMM needs hidden and q/k/v widths in multiples of 256";
    if (c.lm_weight_dtype == 2 && ((c.t_inter + 63) / 64 * 64) % 128)
        return "lm_weight_dtype 2: the MX activation quantiser needs the padded intermediate size (t_inter rounded up to 64) in multiples of 128";
    if (c.v_weight_dtype != 0 && c.v_weight_dtype != 2)
        return "v_weight_dtype 0 (bf16) or 2 (fp8 e4m3 weights x MX fp8 activations on the block-scaled MFMA); v_weight_dtype 1 (fp8 weights under bf16 "
               "activations) exists for a decode weight stream and the vision tower has none";
    if (c.v_weight_dtype == 2) {
        // every K the tower's MX GEMMs see must be whole 128-wide k-tiles, every N whole 256-column tiles (q | k | v sections on tile boundaries)
        static thread_local char why[256];
        const int ip = (c.v_inter + 63) / 64 * 64, mh = c.v_hidden * c.v_merge * c.v_merge;
        const struct { const char* what; int v, mult; } need[] = {
            {"vision hidden_size (K of qkv / gate / up, N of proj / down, q | k | v sections)", c.v_hidden, 256},
            {"vision intermediate_size padded to 64 (K of down_proj)", ip, 128},
            {"vision hidden_size x merge^2 (K and N of merger.mlp.0, K of merger.mlp.2)", mh, 256},
            {"vision out_hidden_size (N of merger.mlp.2)", c.v_out_hidden, 256}};
        for (const auto& n : need)
            if (n.v % n.mult) {
                snprintf(why, sizeof why, "v_weight_dtype 2: %s = %d is not a multiple of %d (the block-scaled fp8 GEMM takes K in 128-wide k-tiles and N in "
                         "256-column tiles)", n.what, n.v, n.mult);
                return why;
            }
        if (ip < 256) return "v_weight_dtype 2: vision intermediate_size padded to 64 must be at least 256 (two 128-wide k-tiles)";
    }
    if (c.max_patches < 4 || c.max_patches % 4 || c.max_prefill_tokens < 1 || c.max_new_tokens < 1) return "capacities";
    if (c.v_n_fullatt < 0 || c.v_n_fullatt > 16 || c.v_depth < 1 || c.t_layers < 1) return "depths";
    return nullptr;
}

// Carves every buffer.  With ar.base == nullptr this is a dry run that only measures.
void carve(sr_engine* e) {
    const sr_config& c = e->c;
    Arena& ar = e->ar;
    e->v_hd = c.v_hidden / c.v_heads;
    e->v_paired = (e->v_hd / 2) % 8 == 0 && e->v_hd % 16 == 0;
    e->v_pd = c.v_in_ch * c.v_temporal * c.v_patch * c.v_patch;
    e->v_pd_pad = rup(e->v_pd, 64);
    e->v_inter_pad = rup(c.v_inter, 64);
    e->v_mh = c.v_hidden * c.v_merge * c.v_merge;
    e->t_inter_pad = rup(c.t_inter, 64);
    e->t_qn = (c.t_heads + 2 * c.t_kv_heads) * 128;
    e->t_group = c.t_heads / c.t_kv_heads;
    e->ks_down = (e->t_inter_pad / 64 >= 16) ? 2 : 1;          // batches above 16 use 4 slabs (32-row GEMV variant)
    e->n_part = gemv_f32_blocks(c.t_vocab, 1, c.t_hidden, 1);   // upper bound (16-row tiles); per-launch count below
    const int C = c.v_hidden, H = c.t_hidden;

    e->weights_begin = (ar.off + 255) & ~(size_t)255;
    e->patch_w = ar.take<bf16_t>((size_t)C * e->v_pd_pad);
    e->vb.resize(c.v_depth);
    for (auto& b : e->vb) {
        b.norm1 = ar.take<bf16_t>(C);
        b.qkv_w = ar.take<bf16_t>((size_t)3 * C * C);
        b.qkv_b = ar.take<bf16_t>(3 * C);
        b.proj_w = ar.take<bf16_t>((size_t)C * C);
        b.proj_b = ar.take<bf16_t>(C);
        b.norm2 = ar.take<bf16_t>(C);
        b.gu_w = ar.take<bf16_t>((size_t)2 * e->v_inter_pad * C);
        b.gu_b = ar.take<bf16_t>(2 * e->v_inter_pad);
        b.down_w = ar.take<bf16_t>((size_t)C * e->v_inter_pad);
        b.down_b = ar.take<bf16_t>(C);
    }
    e->ln_q = ar.take<bf16_t>(C);
    e->fc1_w = ar.take<bf16_t>((size_t)e->v_mh * e->v_mh);
    e->fc1_b = ar.take<bf16_t>(e->v_mh);
    e->fc2_w = ar.take<bf16_t>((size_t)c.v_out_hidden * e->v_mh);
    e->fc2_b = ar.take<bf16_t>(c.v_out_hidden);
    e->embed = ar.take<bf16_t>((size_t)c.t_vocab * H);
    e->final_norm = ar.take<bf16_t>(H);
    e->ll.resize(c.t_layers);
    for (auto& l : e->ll) {
        l.ln1 = ar.take<bf16_t>(H);
        l.qkv_w = ar.take<bf16_t>((size_t)e->t_qn * H);
        l.qkv_b = ar.take<bf16_t>(e->t_qn);
        l.o_w = ar.take<bf16_t>((size_t)H * c.t_heads * 128);
        l.ln2 = ar.take<bf16_t>(H);
        l.gu_w = ar.take<bf16_t>((size_t)2 * e->t_inter_pad * H);
        l.down_w = ar.take<bf16_t>((size_t)H * e->t_inter_pad);
        if (c.lm_weight_dtype >= 1) {
            l.qkv_w8 = ar.take<unsigned char>((size_t)e->t_qn * H);
            l.o_w8 = ar.take<unsigned char>((size_t)H * c.t_heads * 128);
            l.gu_w8 = ar.take<unsigned char>((size_t)2 * e->t_inter_pad * H);
            l.down_w8 = ar.take<unsigned char>((size_t)H * e->t_inter_pad);
            l.qkv_s = ar.take<float>(e->t_qn);
            l.o_s = ar.take<float>(H);
            l.gu_s = ar.take<float>(2 * e->t_inter_pad);
            l.down_s = ar.take<float>(H);
        }
    }
    e->lut = ar.take<bf16_t>(3 * 256);
    e->inv_freq = ar.take<float>(64);
    e->rope_cos = ar.take<bf16_t>((size_t)(c.max_ctx + 1) * 64);
    e->rope_sin = ar.take<bf16_t>((size_t)(c.max_ctx + 1) * 64);
    if (c.v_weight_dtype == 2) {
        for (auto& b : e->vb) {
            b.qkv_w8 = ar.take<unsigned char>((size_t)3 * C * C);
            b.proj_w8 = ar.take<unsigned char>((size_t)C * C);
            b.gu_w8 = ar.take<unsigned char>((size_t)2 * e->v_inter_pad * C);
            b.down_w8 = ar.take<unsigned char>((size_t)C * e->v_inter_pad);
            b.qkv_s = ar.take<float>(3 * C);
            b.proj_s = ar.take<float>(C);
            b.gu_s = ar.take<float>(2 * e->v_inter_pad);
            b.down_s = ar.take<float>(C);
        }
        e->fc1_w8 = ar.take<unsigned char>((size_t)e->v_mh * e->v_mh);
        e->fc2_w8 = ar.take<unsigned char>((size_t)c.v_out_hidden * e->v_mh);
        e->fc1_s = ar.take<float>(e->v_mh);
        e->fc2_s = ar.take<float>(c.v_out_hidden);
    }
    e->weights_end = ar.off;

    // ViT activations
    const size_t NP = c.max_patches;
    e->v_pix = ar.take<bf16_t>(NP * e->v_pd_pad);
    e->v_x = ar.take<bf16_t>(NP * C);
    e->v_xn = ar.take<bf16_t>(NP * C);
    e->v_qkv = ar.take<bf16_t>(NP * 3 * C);
    e->v_attn = ar.take<bf16_t>(NP * C);
    e->v_act = ar.take<bf16_t>(NP * e->v_inter_pad);
    e->v_vt_stride = rup((int)NP, 64) + 64;
    e->v_vt = ar.take<bf16_t>((size_t)C * e->v_vt_stride);
    e->v_m1 = ar.take<bf16_t>(NP / 4 * e->v_mh);
    e->v_cos = ar.take<float>(NP * (e->v_hd / 2));
    e->v_sin = ar.take<float>(NP * (e->v_hd / 2));
    e->v_rowmap_embed = ar.take<int>(NP);
    e->v_rowmap_merge = ar.take<int>(NP / 4);
    e->v_work_win = ar.take<AttnWork>(NP / 4 + 64);
    e->v_work_full = ar.take<AttnWork>(NP / 64 + 64);
    e->v_work_full128 = ar.take<AttnWork>(NP / 128 + 64);
    if (c.v_weight_dtype == 2) {      // sized by max_patches: [NP][C], [NP][inter_pad] and the merged [NP / 4][4 C] all fit NP * max(C, inter_pad) bytes
        e->v_rows_pad = (int)((NP + 255) / 256 * 256);
        const size_t kmax = std::max((size_t)e->v_inter_pad, (size_t)C);
        e->v_q8 = ar.take<unsigned char>(NP * kmax);
        e->v_qs_bytes = (std::max(kmax, (size_t)e->v_mh) / 128 + 1) * (size_t)e->v_rows_pad * 4;
        e->v_qs = ar.take<unsigned char>(e->v_qs_bytes);
    }

    // LM prefill activations
    const size_t TP = c.max_prefill_tokens;
    e->t_x = ar.take<bf16_t>(TP * H);
    e->t_xn = ar.take<bf16_t>(TP * H);
    e->t_qkv = ar.take<bf16_t>(TP * e->t_qn);
    e->t_attn = ar.take<bf16_t>(TP * c.t_heads * 128);
    e->t_act = ar.take<bf16_t>(TP * e->t_inter_pad);
    if (c.lm_weight_dtype == 2) {      // MX activations of the fp8 x fp8 prefill GEMMs: element bytes + e8m0 block scales [K/128][rows_pad][4]
        e->t_rows_pad = (int)((TP + 255) / 256 * 256);
        const size_t kmax = std::max((size_t)e->t_inter_pad, std::max((size_t)H, (size_t)c.t_heads * 128));
        e->t_q8 = ar.take<unsigned char>(TP * kmax);
        e->t_qs = ar.take<unsigned char>((kmax / 128 + 1) * (size_t)e->t_rows_pad * 4);
    }
    e->t_src = ar.take<int>(TP);
    e->t_pos3 = ar.take<int>(3 * TP);
    e->t_slot = ar.take<int>(TP);
    e->t_idx = ar.take<int>(TP);
    e->t_lastrow = ar.take<int>(MAXB);
    e->t_work = ar.take<AttnWork>(TP / 64 + 64);
    e->t_slabs = ar.take<float>((size_t)SPLITK_KS * std::min<size_t>(TP, SPLITK_ROWS) * c.t_hidden);

    // decode
    const size_t B = c.max_batch;
    e->d_xa = ar.take<bf16_t>(B * H);
    e->d_xb = ar.take<bf16_t>(B * H);
    const size_t Bp = (B + 15) / 16 * 16;           // the fragment-ordered x buffers of the batch > 4 decode path hold whole 16-row groups
    e->d_xn = ar.take<bf16_t>(Bp * H);
    e->d_qkv = ar.take<bf16_t>(B * e->t_qn);
    e->d_attn = ar.take<bf16_t>(Bp * c.t_heads * 128);
    e->d_act = ar.take<bf16_t>(Bp * e->t_inter_pad);
    e->d_scores = ar.take<bf16_t>(B * c.t_heads * (size_t)c.max_ctx);
    e->d_logits = ar.take<float>(B * c.t_vocab);
    e->d_slabs = ar.take<float>(4 * B * H);
    e->d_amax_val = ar.take<float>(B * e->n_part);
    e->d_amax_idx = ar.take<int>(B * e->n_part);
    e->d_logits_adm = ar.take<float>(B * c.t_vocab);
    e->d_amax_val_adm = ar.take<float>(B * e->n_part);
    e->d_amax_idx_adm = ar.take<int>(B * e->n_part);
    e->d_row_limit = ar.take<int>(MAXB);
    e->d_row_cs = ar.take<float>(MAXB * 128);
    e->d_px = ar.take<unsigned>(256);
    e->d_ngen = ar.take<int>(MAXB);
    e->d_adm = ar.take<int>(5 * MAXB);
    e->d_adm_slots = ar.take<int>(MAXB);
    e->d_xadm = ar.take<bf16_t>(B * H);           // admission scratch of its own: an admission may run on another stream while rows decode
    e->d_xadm_n = ar.take<bf16_t>((size_t)std::max<size_t>(32, Bp) * H);      // (the admission's 32-row LM-head GEMV addresses two 16-row groups whatever the batch)
    e->d_sampled = ar.take<long long>(MAXB);
    e->d_adm_pick = ar.take<long long>(MAXB);
    e->seen_words = (c.t_vocab + 31) / 32;
    e->d_seen = ar.take<unsigned>((size_t)MAXB * e->seen_words);
    e->d_chosen = ar.take<long long>(MAXB);
    e->d_next = ar.take<long long>(MAXB);
    e->d_cur_tok = ar.take<int>(MAXB);
    e->d_ctx_len = ar.take<int>(MAXB);
    e->d_pos = ar.take<int>(MAXB);
    e->d_finished = ar.take<int>(MAXB);
    e->d_step = ar.take<int>(MAXB);
    e->d_slots = ar.take<int>(MAXB);
    e->d_eos = ar.take<int>(32);
    e->d_tokens = ar.take<int>(B * c.max_new_tokens);
    e->n_slots = c.kv_slots ? c.kv_slots : c.max_batch;
    e->kv_layer_elems = (size_t)e->n_slots * c.t_kv_heads * (size_t)c.max_ctx * 128;
    e->kcache = ar.take<bf16_t>(e->kv_layer_elems * c.t_layers);
    e->vtcache = ar.take<bf16_t>(e->kv_layer_elems * c.t_layers);

    // control staging: ViT needs NP*(8 + 4*hd) + work lists; prefill needs ~24 B per token + work lists
    e->stage_bytes = NP * (8 + 4 * (size_t)e->v_hd) + (NP / 4 + NP / 64 + NP / 128 + 192) * sizeof(AttnWork) + TP * 28 +
                     (TP / 64 + 64) * sizeof(AttnWork) + 4096 + 10 * MAXB * sizeof(int);
    e->d_stage = ar.take<char>(e->stage_bytes);
    e->d_fan = ar.take<int>(5 * MAXB);
}

void register_expected(sr_engine* e) {
    const sr_config& c = e->c;
    char n[160];
    auto add = [&](const char* s) { e->loaded[s] = false; };
    add("visual.patch_embed.proj.weight");
    for (int i = 0; i < c.v_depth; ++i)
        for (const char* s : {"norm1.weight", "norm2.weight", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
                              "attn.proj.bias", "mlp.gate_proj.weight", "mlp.gate_proj.bias", "mlp.up_proj.weight",
                              "mlp.up_proj.bias", "mlp.down_proj.weight", "mlp.down_proj.bias"}) {
            snprintf(n, sizeof n, "visual.blocks.%d.%s", i, s);
            add(n);
        }
    for (const char* s : {"visual.merger.ln_q.weight", "visual.merger.mlp.0.weight", "visual.merger.mlp.0.bias",
                          "visual.merger.mlp.2.weight", "visual.merger.mlp.2.bias", "model.embed_tokens.weight",
                          "model.norm.weight"})
        add(s);
    for (int i = 0; i < c.t_layers; ++i)
        for (const char* s : {"input_layernorm.weight", "post_attention_layernorm.weight", "self_attn.q_proj.weight",
                              "self_attn.q_proj.bias", "self_attn.k_proj.weight", "self_attn.k_proj.bias",
                              "self_attn.v_proj.weight", "self_attn.v_proj.bias", "self_attn.o_proj.weight",
                              "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight"}) {
            snprintf(n, sizeof n, "model.layers.%d.%s", i, s);
            add(n);
        }
}

// waits until the previous control upload has left the pinned staging buffer
int stage_begin(sr_engine* e) {
    if (e->copy_pending) {
        hipError_t r = hipEventSynchronize(e->ev_copy);
        if (r != hipSuccess) return (int)r;
        e->copy_pending = false;
    }
    return 0;
}
int stage_upload(sr_engine* e, size_t off, size_t bytes, hipStream_t s) {
    hipError_t r = hipMemcpyAsync(e->d_stage + off, e->h_stage + off, bytes, hipMemcpyHostToDevice, s);
    if (r != hipSuccess) return (int)r;
    r = hipEventRecord(e->ev_copy, s);
    if (r != hipSuccess) return (int)r;
    e->copy_pending = true;
    return 0;
}

// ------------------------------------------------------------------------------------------------ ViT control data
// window index / cu_seqlens / rotary tables: hf vision_utils.get_vision_window_index (transformers/vision_utils.py:130-188),
// get_vision_position_ids, Qwen2_5_VisionRotaryEmbedding (hf:125-134), written from the definitions.
int vit_prepare(sr_engine* e, const int64_t* grid, int n_img, hipStream_t s, int* n_rows_out) {
    const sr_config& c = e->c;
    int N = 0;
    for (int i = 0; i < n_img; ++i) {
        if (grid[3 * i] != 1) return fail(e, -22, "grid t must be 1 (images only)");
        const int h = (int)grid[3 * i + 1], w = (int)grid[3 * i + 2];
        if (h <= 0 || w <= 0 || h % c.v_merge || w % c.v_merge) return fail(e, -22, "grid h,w must be multiples of merge");
        N += h * w;
    }
    if (N > c.max_patches) return fail(e, -22, "%d patches exceed max_patches %d", N, c.max_patches);
    *n_rows_out = N;
    std::vector<int64_t> key(grid, grid + 3 * n_img);
    if (key == e->v_grid_cached) return 0;

    SR_TRY(stage_begin(e));
    const int half = e->v_hd / 2, nf = half / 2;        // 40 rotary values per row = 20 h-freqs + 20 w-freqs
    const int mg = c.v_merge, unit = mg * mg;
    const int ws = c.v_window / mg / c.v_patch;          // window side in merged units (4)
    std::vector<float> inv(nf);
    for (int i = 0; i < nf; ++i) inv[i] = (float)(1.0 / pow(10000.0, (double)(2 * i) / (double)half));

    char* hp = e->h_stage;
    float* h_cos = reinterpret_cast<float*>(hp);
    float* h_sin = h_cos + (size_t)N * half;
    int* h_rm_embed = reinterpret_cast<int*>(h_sin + (size_t)N * half);
    int* h_rm_merge = h_rm_embed + N;
    AttnWork* h_win = reinterpret_cast<AttnWork*>(((uintptr_t)(h_rm_merge + N / unit) + 15) & ~(uintptr_t)15);
    int n_win = 0;
    std::vector<AttnWork> full, full128;
    bool aligned = true;         // every image starts on a multiple of 8 patches: 16-byte aligned V^T key runs (k_attn_prefill2's LDS-DMA)
    bool all64 = true;           // every window holds exactly 64 tokens (k_attn_win64)

    int unit_base = 0, row_base = 0, new_unit = 0;
    for (int im = 0; im < n_img; ++im) {
        const int gh = (int)grid[3 * im + 1], gw = (int)grid[3 * im + 2];
        const int lh = gh / mg, lw = gw / mg;
        const int nh = (lh + (ws - lh % ws)) / ws, nw = (lw + (ws - lw % ws)) / ws;   // HF pads a full window when aligned
        for (int wy = 0; wy < nh; ++wy)
            for (int wx = 0; wx < nw; ++wx) {
                const int start_unit = new_unit;
                for (int iy = 0; iy < ws; ++iy)
                    for (int ix = 0; ix < ws; ++ix) {
                        const int uy = wy * ws + iy, ux = wx * ws + ix;
                        if (uy >= lh || ux >= lw) continue;
                        const int old_unit = unit_base + uy * lw + ux;
                        h_rm_merge[new_unit] = old_unit;                      // merger output row of window-order unit
                        for (int k = 0; k < unit; ++k) {
                            const int old_row = old_unit * unit + k, new_row = new_unit * unit + k;
                            h_rm_embed[old_row] = new_row;
                            const int py = uy * mg + k / mg, px = ux * mg + k % mg;     // patch (h, w) position
                            for (int f = 0; f < nf; ++f) {
                                const float ah = (float)py * inv[f], aw = (float)px * inv[f];
                                h_cos[(size_t)new_row * half + f] = cosf(ah);
                                h_sin[(size_t)new_row * half + f] = sinf(ah);
                                h_cos[(size_t)new_row * half + nf + f] = cosf(aw);
                                h_sin[(size_t)new_row * half + nf + f] = sinf(aw);
                            }
                        }
                        ++new_unit;
                    }
                const int len = (new_unit - start_unit) * unit;
                // (HF pads one whole extra window row / column when the grid IS a multiple of the window: those windows are empty and make no work item)
                if (len != 0 && (len != 64 || (start_unit * unit) % 4)) all64 = false;
                for (int q0 = 0; q0 < len; q0 += 64)
                    h_win[n_win++] = AttnWork{start_unit * unit + q0, len, q0, start_unit * unit, (long long)start_unit * unit};
            }
        const int len = gh * gw;
        for (int q0 = 0; q0 < len; q0 += 64) full.push_back(AttnWork{row_base + q0, len, q0, row_base, (long long)row_base});
        for (int q0 = 0; q0 < len; q0 += 128) full128.push_back(AttnWork{row_base + q0, len, q0, row_base, (long long)row_base});
        if (row_base % 8) aligned = false;
        unit_base += lh * lw;
        row_base += len;
    }
    AttnWork* h_full = h_win + n_win;
    memcpy(h_full, full.data(), full.size() * sizeof(AttnWork));
    AttnWork* h_full128 = h_full + full.size();
    memcpy(h_full128, full128.data(), full128.size() * sizeof(AttnWork));
    const size_t total = reinterpret_cast<char*>(h_full128 + full128.size()) - hp;
    if (total > e->stage_bytes) return fail(e, -12, "control staging too small");
    SR_TRY(stage_upload(e, 0, total, s));
    // device-side views into the mirror; copied out so that later prefill uploads cannot clobber them
    auto dmirror = [&](const void* hptr) { return e->d_stage + (reinterpret_cast<const char*>(hptr) - hp); };
    SR_TRY((int)hipMemcpyAsync(e->v_cos, dmirror(h_cos), (size_t)N * half * 4, hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->v_sin, dmirror(h_sin), (size_t)N * half * 4, hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->v_rowmap_embed, dmirror(h_rm_embed), (size_t)N * 4, hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->v_rowmap_merge, dmirror(h_rm_merge), (size_t)N / unit * 4, hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->v_work_win, dmirror(h_win), n_win * sizeof(AttnWork), hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->v_work_full, dmirror(h_full), full.size() * sizeof(AttnWork), hipMemcpyDeviceToDevice, s));
    e->v_nwork_win = n_win;
    SR_TRY((int)hipMemcpyAsync(e->v_work_full128, dmirror(h_full128), full128.size() * sizeof(AttnWork), hipMemcpyDeviceToDevice, s));
    e->v_nwork_full = (int)full.size();
    e->v_nwork_full128 = (int)full128.size();
    e->v_full_aligned = aligned;
    e->v_win_all64 = all64;
    e->v_grid_cached = key;
    return 0;
}

bool is_fullatt(const sr_config& c, int blk) {
    for (int i = 0; i < c.v_n_fullatt; ++i) if (c.v_fullatt[i] == blk) return true;
    return false;
}

int gemm(sr_engine* e, hipStream_t s, const bf16_t* A, int lda, const bf16_t* W, int M, int N, int K, void* out, int ldo,
         const bf16_t* bias, const bf16_t* resid, const int* rowmap, int epi, int w_tiled = 0, const float* w_scale = nullptr) {
    GemmArgs a{A, lda, W, M, N, K, out, ldo, bias, resid, rowmap, w_tiled, w_scale, 0};
    SR_TRY(launch_gemm(s, a, epi));
    return 0;
}

// Small prefills (one or two tiles: M = 448 .. 1024 rows): the residual GEMMs (o_proj N = 2048 / K = 2048, down N = 2048 / K = 11008) have
// only ceil(M / 64) * 16 = 112 .. 256 output tiles for 256 CUs and the down-projection walks 172 k-tiles in each of them (140 us of the
// 323 us layer at batch 1).  Split over K (gridDim.y = 4, float32 slabs; the RMSNorm launch that follows anyway sums the slabs into the
// residual stream, launch_resid_rmsnorm: no extra launch, same rounding points) the batch-1 prefill takes 8.0 instead of 11.7 ms.
// OPT-IN (SR_SPLITK=1), static prefill only: the split changes the association of the float32 sums, so a prompt prefilled alone would no
// longer get bit for bit the logits it gets inside a larger batch (the 128- and 256-tile kernels accumulate in the same order), and
// through 36 layers of bf16 rounding that is a noise-floor-sized difference (rms 0.03 on the logits, test_small_prefill_split_k_*):
// correct, but it gives up the batch invariance that the continuous-batching and data-parallel tests assert with torch.equal.
bool prefill_splitk(const sr_engine* e, int n_tok) {
    if (sr_switches().splitk != 1) return false;
    return e->c.lm_weight_dtype != 2 && n_tok <= SPLITK_ROWS && e->c.t_hidden <= 2048 && e->c.t_hidden % 512 == 0;
}

// one linear of the LM prefill.  lm_weight_dtype 0 / 1: MFMA GEMM on bf16 operands (mode 1 multiplies the bf16 image of the fp8-quantised
// weights and scales in the epilogue).  Mode 2 (BASELINE.json configs[4] "CDNA4 fp8 MFMA"): the activations are MX-quantised
// (k_quant_mx_act) and multiplied with the fp8 weight image by the block-scaled K = 128 MFMA -- ALWAYS, whatever the row count, so
// that a sequence's result does not depend on what else is in the batch.
int lm_gemm(sr_engine* e, hipStream_t s, const bf16_t* A, int lda, const bf16_t* W, const unsigned char* W8, const float* w_scale, int M,
            int N, int K, void* out, int ldo, const bf16_t* bias, const bf16_t* resid, int epi, const QkvRope* rope = nullptr, bool* fused = nullptr,
            int ksplit = 0) {
    if (e->c.lm_weight_dtype != 2) {
        GemmArgs a{A, lda, W, M, N, K, out, ldo, bias, resid, nullptr, 1, w_scale, 0};
        a.ksplit = ksplit;
        if (rope) {
            a.rope = *rope;
            if (gemm_fuses_lmqkv(a)) { epi = EPI_LMQKV; *fused = true; }
        }
        SR_TRY(launch_gemm(s, a, epi));
        return 0;
    }
    SR_TRY(launch_quant_mx_act(s, A, lda, M, K, e->t_q8, e->t_qs, e->t_rows_pad));
    GemmArgs a{reinterpret_cast<const bf16_t*>(e->t_q8), K, reinterpret_cast<const bf16_t*>(W8), M, N, K, out, ldo, bias, resid, nullptr, 1, w_scale, 256,
               e->t_qs, e->t_rows_pad};
    if (rope) {
        a.rope = *rope;
        if (gemm_fuses_lmqkv(a)) { epi = EPI_LMQKV; *fused = true; }
    }
    SR_TRY(launch_gemm256_mx(s, a, epi));
    return 0;
}

// one linear of the vision tower.  v_weight_dtype 0: the bf16 MFMA GEMM on the row-major master, exactly the launch `gemm` makes.  Mode 2: the
// input is MX-quantised into the tower's own staging buffers (A == nullptr: k_rmsnorm_mx has already left it there) and multiplied with
// the matrix's fp8 image by the block-scaled MFMA -- as in lm_gemm at ANY row count, so that an image's embedding does not depend on what
// else is in the call.
int vit_gemm(sr_engine* e, hipStream_t s, const bf16_t* A, int lda, const bf16_t* W, const unsigned char* W8, const float* w_scale, int M, int N,
             int K, void* out, int ldo, const bf16_t* bias, const bf16_t* resid, const int* rowmap, int epi, const VitRope* vrope = nullptr) {
    if (e->c.v_weight_dtype != 2) return gemm(e, s, A, lda, W, M, N, K, out, ldo, bias, resid, rowmap, epi);
    if (A) SR_TRY(launch_quant_mx_act(s, A, lda, M, K, e->v_q8, e->v_qs, e->v_rows_pad));
    GemmArgs a{reinterpret_cast<const bf16_t*>(e->v_q8), K, reinterpret_cast<const bf16_t*>(W8), M, N, K, out, ldo, bias, resid, rowmap, 1, w_scale, 256,
               e->v_qs, e->v_rows_pad};
    if (vrope) a.vrope = *vrope;
    SR_TRY(launch_gemm256_mx(s, a, epi));
    return 0;
}

GemvArgs gv(const bf16_t* x, int ldx, const bf16_t* W, int M, int N, int K, void* out, int ldo) {
    GemvArgs a{};
    a.x = x; a.ldx = ldx; a.W = W; a.M = M; a.N = N; a.K = K; a.out = out; a.ldo = ldo; a.ksplit = 1;
    a.w_tiled = 1;      // every LM matrix of the engine is stored fragment-ordered
    return a;
}

// RMSNorms (and the pending residual add) live in the prologue of the consuming GEMV for batches <= 4 (a few KB per
// block); for larger batches every block would have to ingest B rows (+ float32 slabs) before it can start, which was
// measured slower than two small RMSNorm launches spread over the chip
bool fused_norms(const sr_engine* e, int B) { return B <= 4 && e->c.t_hidden % 512 == 0; }
// fragment-ordered activations between the launches of the batch > 4 decode layer (x_tiled): needs whole 64-wide k chunks
bool x_tiled_ok(const sr_engine* e) {
    return e->c.t_hidden % 64 == 0 && (e->c.t_heads * 128) % 64 == 0 && e->t_inter_pad % 64 == 0 && e->c.t_hidden <= 2048;
}
int ks_down(const sr_engine* e, int B) { return (B > 16 && e->t_inter_pad / 64 >= 32) ? 4 : e->ks_down; }

// LM head on B rows of `x` (+ optional pending slabs): float32 logits + per-block argmax partials.
// Small batches fuse the final RMSNorm (and the pending residual) into the GEMV prologue.
int enqueue_lm_head(sr_engine* e, int B, bf16_t* x, bf16_t* x_alt, bool pending, hipStream_t s, bool admission = false) {
    const sr_config& c = e->c;
    const int H = c.t_hidden;
    GemvArgs g = gv(x, H, e->embed, B, c.t_vocab, H, admission ? e->d_logits_adm : e->d_logits, c.t_vocab);
    g.amax_val = admission ? e->d_amax_val_adm : e->d_amax_val; g.amax_idx = admission ? e->d_amax_idx_adm : e->d_amax_idx;
    if (fused_norms(e, B)) {
        g.norm_w = e->final_norm; g.eps = c.t_rms_eps;
        if (pending) { g.slabs = e->d_slabs; g.n_slabs = ks_down(e, B); g.x_out = x_alt; }
    } else {
        // batches > 4: the normalised rows are written fragment-ordered, so the GEMV's x loads are 1 KB contiguous
        const int xt = x_tiled_ok(e) ? 1 : 0;
        if (pending) SR_TRY(launch_resid_rmsnorm(s, x, e->d_slabs, ks_down(e, B), e->final_norm, e->d_xn, B, H, c.t_rms_eps, xt));
        else SR_TRY(launch_rmsnorm(s, x, e->final_norm, e->d_xn, B, H, c.t_rms_eps, xt));
        g.x = e->d_xn; g.x_tiled = xt;
        // on a CU-limited stream the decode step's head keeps x in LDS (k_gemv32_hpx: same bits; the admission's own head stays the streaming kernel)
        if (!admission && (e->px_mode || (sr_switches().gemv_xlds & 4))) g.px_counter = e->d_px;
    }
    SR_TRY(launch_gemv(s, g, GV_F32));
    return 0;
}

// one decode forward pass for rows 0..B-1 (device state decides tokens / positions / context lengths).
// 6 launches per layer at batch <= 4 (qkv, attention scores, attention softmax+PV, o_proj, gate/up, down): norms and
// residual adds live in GEMV prologues / epilogues; larger batches add the two RMSNorm launches.
int enqueue_decode_forward(sr_engine* e, int B, hipStream_t s) {
    const sr_config& c = e->c;
    const int H = c.t_hidden, QD = c.t_heads * 128;
    const bool fused = fused_norms(e, B);
    const int xt = (!fused && x_tiled_ok(e)) ? 1 : 0;      // activations handed from launch to launch in fragment order
    // the x-stationary gate/up and down GEMVs (17..32 rows): on a CU-limited stream (sr_rows_set_cus) -- on the whole chip the streaming kernels are 1 % faster per step;
    // bit 2 of SR_GEMV_XLDS: everywhere (A/B and test hook)
    const bool px = e->px_mode || (sr_switches().gemv_xlds & 4);
    bf16_t *x = e->d_xa, *x_alt = e->d_xb;      // k_step gathered the input embedding into d_xa
    bool pending = false;                       // down-projection slabs not yet added to the residual stream
    const float scale = (float)(1.0 / sqrt(128.0));
    for (int l = 0; l < c.t_layers; ++l) {
        const LmLayerW& w = e->ll[l];
        bf16_t* kc = e->kcache + (size_t)l * e->kv_layer_elems;
        bf16_t* vc = e->vtcache + (size_t)l * e->kv_layer_elems;
        GemvArgs gq = gv(x, H, w.qkv_w, B, e->t_qn, H, e->d_qkv, e->t_qn);
        gq.bias = w.qkv_b; gq.W8 = w.qkv_w8; gq.w_scale = w.qkv_s;
        if (fused) {
            gq.norm_w = w.ln1; gq.eps = c.t_rms_eps;
            if (pending) { gq.slabs = e->d_slabs; gq.n_slabs = ks_down(e, B); gq.x_out = x_alt; }
        } else {
            if (pending) SR_TRY(launch_resid_rmsnorm(s, x, e->d_slabs, ks_down(e, B), w.ln1, e->d_xn, B, H, c.t_rms_eps, xt));
            else SR_TRY(launch_rmsnorm(s, x, w.ln1, e->d_xn, B, H, c.t_rms_eps, xt));
            gq.x = e->d_xn; gq.x_tiled = xt;
        }
        SR_TRY(launch_gemv(s, gq, GV_BIAS));
        if (fused && pending) { bf16_t* t = x; x = x_alt; x_alt = t; }     // block 0 wrote the updated stream there
        pending = false;
        DecodeAttnArgs da{e->d_qkv, e->t_qn, e->d_pos, e->d_ctx_len, e->d_slots, e->rope_cos, e->rope_sin, kc, vc, e->d_attn, QD,
                          B, c.t_heads, c.t_kv_heads, e->t_group, c.max_ctx, scale, e->d_scores, xt, e->d_finished, e->d_row_cs};
        SR_TRY(launch_attn_decode(s, da));
        GemvArgs go = gv(e->d_attn, QD, w.o_w, B, H, QD, x, H);
        go.W8 = w.o_w8; go.w_scale = w.o_s; go.x_tiled = xt;
        SR_TRY(launch_gemv(s, go, GV_RESID));
        GemvArgs gg = gv(x, H, w.gu_w, B, 2 * e->t_inter_pad, H, e->d_act, e->t_inter_pad);
        gg.W8 = w.gu_w8; gg.w_scale = w.gu_s;
        if (fused) { gg.norm_w = w.ln2; gg.eps = c.t_rms_eps; }
        else if (B > 64 && !w.gu_w8) {
            // more than 64 rows: gate/up as an LDS-tiled MFMA GEMM (gemm.hip, 64 x 128 tiles: every block stages its x tile ONCE for its four
            // waves).  The row-group GEMV reads G x the weight bytes of x from L2 per wave (43 us at 128 rows; decode step 4.50 -> 4.19 ms with
            // the tile kernel); the other launches keep the GEMV (their narrow matrices would give the tile kernel 32-40 blocks), and at 64 rows
            // the GEMV is as fast (3.24 vs 3.29 ms per step).  Row-major x in, fragment-ordered activation out (the down GEMV's x).
            SR_TRY(launch_rmsnorm(s, x, w.ln2, e->d_xn, B, H, c.t_rms_eps, 0));
            GemmArgs ga{e->d_xn, H, w.gu_w, B, 2 * e->t_inter_pad, H, e->d_act, e->t_inter_pad, nullptr, nullptr, nullptr, 1, nullptr, 128};
            ga.out_tiled = xt;
            SR_TRY(launch_gemm(s, ga, EPI_SWIGLU));
            gg.M = 0;       // (done)
        }
        else {
            SR_TRY(launch_rmsnorm(s, x, w.ln2, e->d_xn, B, H, c.t_rms_eps, xt));
            gg.x = e->d_xn; gg.x_tiled = xt; gg.out_tiled = xt;
            gg.px_counter = px ? e->d_px : nullptr;        // 17..32 rows: launch_gemv may take the persistent x-resident kernel (same bits)
        }
        if (gg.M > 0) SR_TRY(launch_gemv(s, gg, GV_SWIGLU));
        GemvArgs gd = gv(e->d_act, e->t_inter_pad, w.down_w, B, H, e->t_inter_pad, e->d_slabs, H);
        gd.ksplit = ks_down(e, B);
        gd.W8 = w.down_w8; gd.w_scale = w.down_s; gd.x_tiled = xt;
        gd.px_counter = px ? e->d_px : nullptr;            // 17..32 rows, bf16: the x-stationary split-K kernel (same bits)
        SR_TRY(launch_gemv(s, gd, GV_PARTIAL));
        pending = true;
    }
    return enqueue_lm_head(e, B, x, x_alt, pending, s, false);
}

int enqueue_step(sr_engine* e, int B, int n_eos, int pad_id, const int* forced, hipStream_t s, const long long* chosen = nullptr) {
    StepArgs a{e->d_amax_val, e->d_amax_idx, gemv_f32_blocks(e->c.t_vocab, B, e->c.t_hidden, fused_norms(e, B) ? 1 : 0), e->d_cur_tok, e->d_ctx_len, e->d_pos, e->d_step, e->d_finished,
               e->d_tokens, e->c.max_new_tokens, e->d_eos, n_eos, pad_id, B, forced, e->embed, e->d_xa, e->c.t_hidden, 1, chosen, e->d_row_limit, e->d_ngen,
               e->rope_cos, e->rope_sin, e->d_row_cs};
    SR_TRY(launch_step(s, a));
    return 0;
}

// k_sample's arguments for n draws, the engine-constant part: the decode logits at every row's step -> d_sampled, with the LM head's
// block maxima; or (admission) the admission logits -> d_adm_pick.  The scalars start as the placeholders of the per-row table forms
SampleArgs sample_args(const sr_engine* e, int n, bool admission) {
    const sr_config& c = e->c;
    SampleArgs a{};
    a.V = c.t_vocab; a.B = n; a.seen_words = e->seen_words;
    a.inv_temp = 1.0f; a.top_k = 1; a.top_p = 1.0f; a.rep_penalty = 1.0f;
    if (admission) { a.logits = e->d_logits_adm; a.out = e->d_adm_pick; return a; }
    const int hn = fused_norms(e, n) ? 1 : 0;
    a.logits = e->d_logits; a.step = e->d_step; a.out = e->d_sampled;
    a.blk_max = e->d_amax_val; a.n_blk = gemv_f32_blocks(c.t_vocab, n, c.t_hidden, hn); a.blk_rows = gemv_f32_block_rows(c.t_vocab, n, c.t_hidden, hn);
    return a;
}

// ---- one decode step: k_step consumes every row's pending token (log, eos / limit bookkeeping, next input embedding), the forward
// runs, and the tail leaves the next pending tokens where the next k_step reads them.  The captured AND the eager form of every
// variant are enqueue_decode_step on this description
struct Step {
    int B, n_eos, pad_id;
    const int* forced;            // teacher-forced tokens (sr_decode)
    const long long* chosen;      // the pending tokens; null: the arg-max of the LM head's partials
    // repetition-penalty bitmaps, marked with the pending tokens: MARK_ROWS before k_step (rp_seen: per KV slot, unfinished rows),
    // MARK_CHOSEN after it (d_seen: per row)
    enum { MARK_NONE, MARK_ROWS, MARK_CHOSEN } mark;
    enum { TAIL_NONE, TAIL_SAMPLE, TAIL_NEXT_IDS, TAIL_BEAM } tail;
    SampleArgs sample;                                   // TAIL_SAMPLE
    const BeamArgs* beam; const KvSuffixArgs* suffix;    // TAIL_BEAM: row statistics, group select, KV suffix copies
};
Step make_step(int B, int n_eos, int pad_id, const long long* chosen) {
    Step st{};
    st.B = B; st.n_eos = n_eos; st.pad_id = pad_id; st.chosen = chosen;
    return st;
}
// the steps that pick their tokens themselves record log-probs under sr_logprobs (beam search and sr_decode_step do not)
bool step_records(const sr_engine* e, const Step& st) { return e->lp_n >= 0 && (st.tail == Step::TAIL_NONE || st.tail == Step::TAIL_SAMPLE); }
StepKey step_key(const sr_engine* e, const Step& st) {
    StepKey k{};
    k.B = st.B; k.n_eos = st.n_eos; k.pad_id = st.pad_id;
    k.lp = step_records(e, st) ? e->lp_n + 1 : 0;
    if (st.tail == Step::TAIL_SAMPLE) {
        k.top_k = st.sample.top_k; k.inv_temp = st.sample.inv_temp; k.top_p = st.sample.top_p; k.rep_penalty = st.sample.rep_penalty; k.seed = st.sample.seed;
    } else if (st.tail == Step::TAIL_BEAM) {      // (k_step runs without eos there: the select kernel owns them)
        k.n_eos = st.beam->n_eos; k.W = st.beam->W; k.K = st.beam->K; k.max_new = st.beam->max_new; k.length_penalty = st.beam->lp;
    }
    return k;
}

int enqueue_step_tail(sr_engine* e, const Step& st, hipStream_t q) {
    const sr_config& c = e->c;
    if (st.tail == Step::TAIL_SAMPLE) SR_TRY(launch_sample(q, st.sample));
    if (st.tail == Step::TAIL_NEXT_IDS)
        SR_TRY(launch_next_ids(q, e->d_amax_val, e->d_amax_idx, gemv_f32_blocks(c.t_vocab, st.B, c.t_hidden, fused_norms(e, st.B) ? 1 : 0), st.B, e->d_next));
    if (st.tail == Step::TAIL_BEAM) {
        SR_TRY(launch_beam_rowstats(q, *st.beam));
        SR_TRY(launch_beam_select(q, *st.beam));
        SR_TRY(launch_kv_suffix(q, *st.suffix));
    }
    if (step_records(e, st)) {      // the pending tokens' records, at the log index k_step will give them (live rows only)
        LogprobArgs la{e->d_logits, c.t_vocab, c.t_vocab, st.B, e->lp_n, nullptr, e->lp_part, st.chosen, e->d_step, e->d_finished, c.max_new_tokens,
                       e->lp_log, nullptr, e->lp_ids, e->lp_tlp};
        SR_TRY(launch_logprobs(q, la));
    }
    return 0;
}

// logits_copy: eager traced runs keep the step's float32 logits [B, V]
int enqueue_decode_step(sr_engine* e, const Step& st, hipStream_t q, float* logits_copy = nullptr) {
    if (st.mark == Step::MARK_ROWS) SR_TRY(launch_mark_rows(q, st.chosen, e->d_finished, e->d_slots, e->rp_seen, e->seen_words, st.B));
    if (int rc = enqueue_step(e, st.B, st.n_eos, st.pad_id, st.forced, q, st.chosen)) return rc;
    if (st.mark == Step::MARK_CHOSEN) SR_TRY(launch_mark_chosen(q, st.chosen, e->d_seen, e->seen_words, st.B));
    if (int rc = enqueue_decode_forward(e, st.B, q)) return rc;
    if (logits_copy) SR_TRY((int)hipMemcpyAsync(logits_copy, e->d_logits, (size_t)st.B * e->c.t_vocab * 4, hipMemcpyDeviceToDevice, q));
    return enqueue_step_tail(e, st, q);
}

// The step as a ready graph: slot [kind][px_mode] of the cache, reused while its key matches, otherwise captured again on cap_stream
int step_graph(sr_engine* e, StepKind kind, const Step& st, hipGraphExec_t* exec) {
    StepGraph& sg = e->graphs[kind][e->px_mode];
    const StepKey key = step_key(e, st);
    if (sg.exec == nullptr || memcmp(&sg.key, &key, sizeof key) != 0) {
        if (sg.exec) { (void)hipGraphExecDestroy(sg.exec); sg.exec = nullptr; }
        hipGraph_t g = nullptr;
        SR_TRY((int)hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeRelaxed));
        const int rc = enqueue_decode_step(e, st, e->cap_stream);
        hipError_t er = hipStreamEndCapture(e->cap_stream, &g);
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        SR_TRY((int)er);
        er = hipGraphInstantiate(&sg.exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        SR_TRY((int)er);
        sg.key = key;
    }
    *exec = sg.exec;
    return 0;
}

// The step loop of the static decodes: steps first .. max_new - 1 (replays of `exec`, or eager launches that keep each step's logits
// from `trace` on), stopping once all n_flags device flags are set (read every 16th step; d_flags null: never).  record_last: step
// max_new - 1 only records its token.  -> *done = steps issued, counted from 0
int run_steps(sr_engine* e, const Step& st, hipGraphExec_t exec, int first, int max_new, bool record_last, float* trace, const int* d_flags,
              int n_flags, hipStream_t s, int* done) {
    const size_t BV = (size_t)st.B * e->c.t_vocab;
    std::vector<int> flags(n_flags);
    *done = first;
    for (int i = first; i < max_new; ++i) {
        if (record_last && i == max_new - 1) {
            if (int rc = enqueue_step(e, st.B, st.n_eos, st.pad_id, st.forced, s, st.chosen)) return rc;
            *done = max_new;
            break;
        }
        if (exec) SR_TRY((int)hipGraphLaunch(exec, s));
        else if (int rc = enqueue_decode_step(e, st, s, trace ? trace + (size_t)(i - first) * BV : nullptr)) return rc;
        *done = i + 1;
        if (d_flags && (i % 16) == 15) {
            SR_TRY((int)hipMemcpyAsync(flags.data(), d_flags, n_flags * 4, hipMemcpyDeviceToHost, s));
            SR_TRY((int)hipStreamSynchronize(s));
            bool all = true;
            for (int f : flags) all &= f != 0;
            if (all) break;
        }
    }
    return 0;
}

// sr_decode / sr_decode_sample: the steps (early exit once every sequence has emitted an eos token), then the token log
// [B][max_new_tokens] -> caller layout [B][max_new]; unwritten positions read as pad
int decode_static(sr_engine* e, const Step& st, hipGraphExec_t exec, int max_new, float* trace, int32_t* tokens_out, hipStream_t s, int* steps_done) {
    const sr_config& c = e->c;
    int done = 0;
    if (int rc = run_steps(e, st, exec, 0, max_new, true, trace, st.n_eos ? e->d_finished : nullptr, st.B, s, &done)) return rc;
    if (done < max_new) {
        // fill the tail of the device log with pad before copying out
        std::vector<int> padrow(max_new, st.pad_id);
        for (int b = 0; b < st.B; ++b)
            SR_TRY((int)hipMemcpyAsync(e->d_tokens + (size_t)b * c.max_new_tokens + done, padrow.data(), (max_new - done) * 4, hipMemcpyHostToDevice, s));
        SR_TRY((int)hipStreamSynchronize(s));
    }
    SR_TRY((int)hipMemcpy2DAsync(tokens_out, (size_t)max_new * 4, e->d_tokens, (size_t)c.max_new_tokens * 4, (size_t)max_new * 4, st.B,
                                 hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipStreamSynchronize(s));
    if (steps_done) *steps_done = done;
    return 0;
}

// sr_decode under sr_logprobs: rows 0..B-1 of the log cleared (what the pads after a finished row read as), then the first tokens' records
// from the prefill logits
int begin_static_log(sr_engine* e, const Step& st, hipStream_t s) {
    if (!step_records(e, st)) return 0;
    SR_TRY(launch_logprob_clear(s, st.B * e->c.max_new_tokens, e->lp_log, e->lp_ids, e->lp_tlp));
    return enqueue_step_tail(e, st, s);
}

}  // namespace

// counter block of the x-stationary GEMVs for the op-level entry points (engines own theirs): 8 ticket shards + done count + the CU limit, 64 B apart
static unsigned* g_op_px = nullptr;
static int g_op_px_mode = 0;         // as sr_engine::px_mode: the x-stationary forms after sr_op_gemv_set_cus(n > 0) (or bit 2 of SR_GEMV_XLDS)
static int op_px() {
    if (g_op_px) return 0;
    if (hipMalloc(&g_op_px, 256 * sizeof(unsigned)) != hipSuccess || hipMemset(g_op_px, 0, 256 * sizeof(unsigned)) != hipSuccess) return -12;
    return 0;
}

// =================================================================================================== C ABI
extern "C" {

int sr_version(void) { return 1; }

int sr_switches_reload(void) { load_switches(); return 0; }

const char* sr_last_error(const sr_engine* e) { return e ? e->err : g_err; }

size_t sr_workspace_bytes(const sr_config* cfg) {
    if (!cfg) return 0;
    if (const char* why = validate(*cfg)) { (void)fail(nullptr, -22, "invalid sr_config: %s", why); return 0; }
    sr_engine tmp;
    tmp.c = *cfg;
    carve(&tmp);
    return tmp.ar.off + 4096;
}

int sr_engine_create(const sr_config* cfg, void* workspace, size_t workspace_bytes, sr_engine** out) {
    if (!cfg || !workspace || !out) return fail(nullptr, -22, "null argument");
    if (const char* why = validate(*cfg)) return fail(nullptr, -22, "invalid sr_config: %s", why);
    if ((uintptr_t)workspace & 255) return fail(nullptr, -22, "workspace must be 256-byte aligned");
    sr_engine* e = new sr_engine();
    e->c = *cfg;
    load_switches();                            // the environment is read here (and by sr_switches_reload), never in per-call dispatch
    snprintf(e->err, sizeof e->err, "ok");
    {   // the engine belongs to the device that owns the workspace, whatever the calling thread's current device is
        hipPointerAttribute_t pa{};
        int cur = 0;
        (void)hipGetDevice(&cur);
        e->device = (hipPointerGetAttributes(&pa, workspace) == hipSuccess) ? pa.device : cur;
        (void)hipGetLastError();
        (void)hipSetDevice(e->device);
    }
    e->ar.base = static_cast<char*>(workspace);
    e->ar.cap = workspace_bytes;
    carve(e);
    if (e->ar.off > workspace_bytes) {
        size_t need = e->ar.off;
        delete e;
        return fail(nullptr, -12, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    }
    register_expected(e);
    hipError_t r = hipHostMalloc(reinterpret_cast<void**>(&e->h_stage), e->stage_bytes, hipHostMallocDefault);
    if (r != hipSuccess) { delete e; return fail(nullptr, (int)r, "hipHostMalloc: %s", hipGetErrorString(r)); }
    r = hipEventCreateWithFlags(&e->ev_copy, hipEventDisableTiming);
    if (r != hipSuccess) { (void)hipHostFree(e->h_stage); delete e; return fail(nullptr, (int)r, "hipEventCreate"); }
    r = hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking);
    if (r != hipSuccess) { (void)hipEventDestroy(e->ev_copy); (void)hipHostFree(e->h_stage); delete e; return fail(nullptr, (int)r, "hipStreamCreate"); }
    // zero weights (padding must be 0), KV cache (0 * stale must stay finite) and decode state
    r = hipMemset(e->ar.base + e->weights_begin, 0, e->weights_end - e->weights_begin);
    if (r == hipSuccess) r = hipMemset(e->kcache, 0, e->kv_layer_elems * e->c.t_layers * sizeof(bf16_t));
    if (r == hipSuccess) r = hipMemset(e->vtcache, 0, e->kv_layer_elems * e->c.t_layers * sizeof(bf16_t));
    if (r == hipSuccess) r = hipMemset(e->d_cur_tok, 0, (char*)e->d_tokens - (char*)e->d_cur_tok);
    if (r == hipSuccess) r = hipMemset(e->d_px, 0, 256 * sizeof(unsigned));
    if (r == hipSuccess) r = hipMemset(e->v_vt, 0, (size_t)e->c.v_hidden * e->v_vt_stride * sizeof(bf16_t));
    // (the GEMM reads the scale rows of a whole 256-row tile: rows past the call's last stay valid e8m0 bytes, their products finite)
    if (r == hipSuccess && e->v_qs) r = hipMemset(e->v_qs, 0, e->v_qs_bytes);
    // normalise LUT (hf image_transforms.py:89-124, 384-440) and rotary inverse frequencies (hf:506-523)
    std::vector<bf16_t> lut(768);
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    for (int ch = 0; ch < 3; ++ch)
        for (int u = 0; u < 256; ++u) {
            const float x = (float)((double)u * (1.0 / 255.0));
            lut[ch * 256 + u] = host_f2bf((x - mean[ch]) / stdv[ch]);
        }
    std::vector<float> inv(64);
    for (int i = 0; i < 64; ++i) inv[i] = (float)(1.0 / pow((double)e->c.t_rope_theta, (double)(2 * i) / 128.0));
    if (r == hipSuccess) r = hipMemcpy(e->lut, lut.data(), 768 * sizeof(bf16_t), hipMemcpyHostToDevice);
    if (r == hipSuccess) r = hipMemcpy(e->inv_freq, inv.data(), 64 * sizeof(float), hipMemcpyHostToDevice);
    if (r == hipSuccess) r = (hipError_t)launch_rope_table(nullptr, e->inv_freq, e->c.max_ctx + 1, e->rope_cos, e->rope_sin);
    if (r == hipSuccess) r = hipDeviceSynchronize();
    if (r == hipSuccess) r = (hipError_t)attn_decode_prepare(e->c.max_ctx, e->t_group);
    if (r == hipSuccess && e->c.max_batch > 64) r = (hipError_t)gemm_prepare_decode();
    if (r == hipSuccess) r = (hipError_t)gemv_prepare_px();
    if (r != hipSuccess) {
        int rc = fail(nullptr, (int)r, "engine init: %s", hipGetErrorString(r));
        sr_engine_destroy(e);
        return rc;
    }
    *out = e;
    return 0;
}

int sr_engine_destroy(sr_engine* e) {
    enter(e);
    if (!e) return 0;
    for (auto& kind : e->graphs) for (auto& g : kind) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (e->beam_mem) (void)hipFree(e->beam_mem);
    if (e->rp_mem) (void)hipFree(e->rp_mem);
    if (e->lp_mem) (void)hipFree(e->lp_mem);
    if (e->h_rp) (void)hipHostFree(e->h_rp);
    if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
    if (e->ev_copy) (void)hipEventDestroy(e->ev_copy);
    if (e->h_stage) (void)hipHostFree(e->h_stage);
    delete e;
    return 0;
}

int sr_weights_missing(const sr_engine* e, char* first_missing, size_t cap) {
    int n = 0;
    for (const auto& kv : e->loaded)
        if (!kv.second) {
            if (n == 0 && first_missing && cap) snprintf(first_missing, cap, "%s", kv.first.c_str());
            ++n;
        }
    return n;
}

int sr_synth_fill(void* dev_out_bf16, int64_t n, const char* hf_name, uint32_t seed, float base, void* stream) {
    const uint32_t key = mix32h(fnv1a32(hf_name) ^ mix32h(seed + 0x9E3779B9u));
    int rc = launch_synth_fill((hipStream_t)stream, (bf16_t*)dev_out_bf16, n, key, base, 1.3531647e-4f);
    if (rc) return fail(nullptr, rc, "synth_fill launch failed (%d)", rc);
    return 0;
}

int sr_load_weight(sr_engine* e, const char* hf_name, const void* p, int dtype, const int64_t* shape, int ndim, void* stream) {
    enter(e);
    if (!e || !hf_name || !p || !shape || ndim < 1) return fail(e, -22, "sr_load_weight: null argument");
    if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return fail(e, -22, "sr_load_weight: dtype");
    hipStream_t s = (hipStream_t)stream;
    const sr_config& c = e->c;
    std::string name = hf_name;
    if (name.rfind("model.visual.", 0) == 0) name = name.substr(6);
    else if (name.rfind("model.language_model.", 0) == 0) name = "model." + name.substr(21);
    if (name == "lm_head.weight") return 0;   // tied to model.embed_tokens.weight
    long long rows = shape[0], cols = 1;
    for (int i = 1; i < ndim; ++i) cols *= shape[i];
    const int C = c.v_hidden, H = c.t_hidden;
    bf16_t* dst = nullptr;
    long long ld = cols, exp_rows = -1, exp_cols = -1, row_off = 0;
    int mode = 0, tiled = 0;
    int idx = -1;
    char sub[96] = "";
    if (name == "visual.patch_embed.proj.weight") { dst = e->patch_w; ld = e->v_pd_pad; exp_rows = C; exp_cols = e->v_pd; }
    else if (sscanf(name.c_str(), "visual.blocks.%d.%95s", &idx, sub) == 2 && idx >= 0 && idx < c.v_depth) {
        VitBlockW& b = e->vb[idx];
        const std::string t = sub;
        if (t == "norm1.weight") { dst = b.norm1; exp_rows = C; exp_cols = 1; }
        else if (t == "norm2.weight") { dst = b.norm2; exp_rows = C; exp_cols = 1; }
        // q / k channels of every head in paired order (vit_qk_perm): rotary partners 8 apart inside one 16-column tile
        else if (t == "attn.qkv.weight") { dst = b.qkv_w; exp_rows = 3 * C; exp_cols = C; if (e->v_paired) { mode = 3; row_off = e->v_hd; } b.dirty[0] = 1; }
        else if (t == "attn.qkv.bias") { dst = b.qkv_b; exp_rows = 3 * C; exp_cols = 1; if (e->v_paired) { mode = 3; row_off = e->v_hd; } }
        else if (t == "attn.proj.weight") { dst = b.proj_w; exp_rows = C; exp_cols = C; b.dirty[1] = 1; }
        else if (t == "attn.proj.bias") { dst = b.proj_b; exp_rows = C; exp_cols = 1; }
        else if (t == "mlp.gate_proj.weight") { dst = b.gu_w; exp_rows = c.v_inter; exp_cols = C; mode = 1; b.dirty[2] = 1; }
        else if (t == "mlp.gate_proj.bias") { dst = b.gu_b; exp_rows = c.v_inter; exp_cols = 1; mode = 1; }
        else if (t == "mlp.up_proj.weight") { dst = b.gu_w; exp_rows = c.v_inter; exp_cols = C; mode = 2; b.dirty[2] = 1; }
        else if (t == "mlp.up_proj.bias") { dst = b.gu_b; exp_rows = c.v_inter; exp_cols = 1; mode = 2; }
        else if (t == "mlp.down_proj.weight") { dst = b.down_w; exp_rows = C; exp_cols = c.v_inter; ld = e->v_inter_pad; b.dirty[3] = 1; }
        else if (t == "mlp.down_proj.bias") { dst = b.down_b; exp_rows = C; exp_cols = 1; }
    }
    else if (name == "visual.merger.ln_q.weight") { dst = e->ln_q; exp_rows = C; exp_cols = 1; }
    else if (name == "visual.merger.mlp.0.weight") { dst = e->fc1_w; exp_rows = e->v_mh; exp_cols = e->v_mh; e->fc_dirty[0] = 1; }
    else if (name == "visual.merger.mlp.0.bias") { dst = e->fc1_b; exp_rows = e->v_mh; exp_cols = 1; }
    else if (name == "visual.merger.mlp.2.weight") { dst = e->fc2_w; exp_rows = c.v_out_hidden; exp_cols = e->v_mh; e->fc_dirty[1] = 1; }
    else if (name == "visual.merger.mlp.2.bias") { dst = e->fc2_b; exp_rows = c.v_out_hidden; exp_cols = 1; }
    else if (name == "model.embed_tokens.weight") { dst = e->embed; exp_rows = c.t_vocab; exp_cols = H; tiled = 1; }
    else if (name == "model.norm.weight") { dst = e->final_norm; exp_rows = H; exp_cols = 1; }
    else if (sscanf(name.c_str(), "model.layers.%d.%95s", &idx, sub) == 2 && idx >= 0 && idx < c.t_layers) {
        LmLayerW& l = e->ll[idx];
        const std::string t = sub;
        const int QD = c.t_heads * 128, KD = c.t_kv_heads * 128;
        int dm = -1, dbit = 0;          // fused matrix + constituent bit of an LM linear weight (fp8 re-quantisation bookkeeping)
        if (t == "input_layernorm.weight") { dst = l.ln1; exp_rows = H; exp_cols = 1; }
        else if (t == "post_attention_layernorm.weight") { dst = l.ln2; exp_rows = H; exp_cols = 1; }
        else if (t == "self_attn.q_proj.weight") { tiled = 1; dst = l.qkv_w; exp_rows = QD; exp_cols = H; dm = 0; dbit = 1; }
        else if (t == "self_attn.q_proj.bias") { dst = l.qkv_b; exp_rows = QD; exp_cols = 1; }
        else if (t == "self_attn.k_proj.weight") { tiled = 1; dst = l.qkv_w; exp_rows = KD; exp_cols = H; row_off = QD; dm = 0; dbit = 2; }
        else if (t == "self_attn.k_proj.bias") { dst = l.qkv_b; exp_rows = KD; exp_cols = 1; row_off = QD; }
        else if (t == "self_attn.v_proj.weight") { tiled = 1; dst = l.qkv_w; exp_rows = KD; exp_cols = H; row_off = QD + KD; dm = 0; dbit = 4; }
        else if (t == "self_attn.v_proj.bias") { dst = l.qkv_b; exp_rows = KD; exp_cols = 1; row_off = QD + KD; }
        else if (t == "self_attn.o_proj.weight") { tiled = 1; dst = l.o_w; exp_rows = H; exp_cols = QD; dm = 1; dbit = 1; }
        else if (t == "mlp.gate_proj.weight") { tiled = 1; dst = l.gu_w; exp_rows = c.t_inter; exp_cols = H; mode = 1; dm = 2; dbit = 1; }
        else if (t == "mlp.up_proj.weight") { tiled = 1; dst = l.gu_w; exp_rows = c.t_inter; exp_cols = H; mode = 2; dm = 2; dbit = 2; }
        else if (t == "mlp.down_proj.weight") { tiled = 1; dst = l.down_w; exp_rows = H; exp_cols = c.t_inter; ld = e->t_inter_pad; dm = 3; dbit = 1; }
        if (dm >= 0 && rows == exp_rows && cols == exp_cols) l.dirty[dm] |= (unsigned char)dbit;
    }
    if (!dst) return fail(e, -2, "sr_load_weight: unknown parameter '%s'", hf_name);
    if (rows != exp_rows || cols != exp_cols)
        return fail(e, -22, "sr_load_weight: '%s' has shape [%lld, %lld], expected [%lld, %lld]", hf_name, rows, cols, exp_rows, exp_cols);
    SR_TRY(launch_load2d(s, p, dtype, rows, cols, dst, ld, mode, row_off, tiled));
    e->loaded[name] = true;
    e->finalized = false;     // fp8 mode: the matrix has to be (re)quantised before the next forward
    return 0;
}

int sr_vit_plan(const sr_engine* e, int32_t* out4) {
    if (!e || !out4) return -22;
    out4[0] = e->v_nwork_win; out4[1] = e->v_nwork_full; out4[2] = e->v_win_all64 ? 1 : 0; out4[3] = e->v_full_aligned ? 1 : 0;
    return 0;
}
int sr_pixel_ld(const sr_engine* e) { return e->v_pd_pad; }

int sr_patchify_u8(sr_engine* e, const uint8_t* img, int h, int w, void* out, void* stream) {
    enter(e);
    const sr_config& c = e->c;
    const int f = c.v_patch * c.v_merge;
    if (c.v_in_ch != 3 || h % f || w % f || h <= 0 || w <= 0) return fail(e, -22, "sr_patchify_u8: h,w must be multiples of %d", f);
    SR_TRY(launch_patchify((hipStream_t)stream, img, h, w, e->lut, (bf16_t*)out, e->v_pd_pad, c.v_patch, c.v_merge, c.v_temporal));
    return 0;
}

int sr_vit_forward(sr_engine* e, const void* pixels, int pixels_dtype, const int64_t* grid, int n_img, void* out, void* stream) {
    enter(e);
    if (!e || !pixels || !grid || !out || n_img < 1) return fail(e, -22, "sr_vit_forward: null argument");
    char miss[160];
    if (sr_weights_missing(e, miss, sizeof miss)) return fail(e, -61, "weights missing, e.g. '%s'", miss);
    hipStream_t s = (hipStream_t)stream;
    const sr_config& c = e->c;
    int N = 0;
    if (int rc = vit_prepare(e, grid, n_img, s, &N)) return rc;
    const int C = c.v_hidden, hd = e->v_hd;
    const bf16_t* pix = static_cast<const bf16_t*>(pixels);
    if (pixels_dtype == SR_DTYPE_F32) {
        SR_TRY(launch_f32_to_bf16_pad(s, static_cast<const float*>(pixels), N, e->v_pd, e->v_pix, e->v_pd_pad));
        pix = e->v_pix;
    } else if (pixels_dtype != SR_DTYPE_BF16) return fail(e, -22, "pixels dtype");
    // patch embed (Conv3d k=s, no bias, hf:99-122) with the window permutation fused into the store (hf:433-441)
    if (int rc = gemm(e, s, pix, e->v_pd_pad, e->patch_w, N, C, e->v_pd_pad, e->v_x, C, nullptr, nullptr, e->v_rowmap_embed, EPI_STORE)) return rc;
    const float scale = (float)(1.0 / sqrt((double)hd));
    const bool mx = c.v_weight_dtype == 2;      // fp8 x fp8 linears: every RMSNorm feeds only a GEMM, so it quantises in the same pass (v_xn is never written)
    if (mx && !e->finalized) return fail(e, -22, "fp8 vision tower: call sr_finalize_weights after loading");
    auto norm = [&](const bf16_t* nw, int group) {
        return mx ? launch_rmsnorm_mx(s, e->v_x, nw, e->v_q8, e->v_qs, N, C, 1e-6f, group, e->v_rows_pad) : launch_rmsnorm(s, e->v_x, nw, e->v_xn, N, C, 1e-6f, 0, 1);
    };
    const bf16_t* xn = mx ? nullptr : e->v_xn;    // vit_gemm: null = the operand is already in v_q8 / v_qs
    for (int blk = 0; blk < c.v_depth; ++blk) {
        const VitBlockW& w = e->vb[blk];
        SR_TRY(norm(w.norm1, 1));
        // qkv Linear; the 2-D rotary embedding and the V transpose ride in the GEMM epilogue when the 256-tile kernel takes the shape
        // (large batches; needs the paired q / k channel order the loader established), else they are the two launches of round 1
        if (mx) {
            const VitRope vr{e->v_cos, e->v_sin, e->v_vt, e->v_vt_stride, C, hd};
            if (int rc = vit_gemm(e, s, nullptr, C, nullptr, w.qkv_w8, w.qkv_s, N, 3 * C, C, e->v_qkv, 3 * C, w.qkv_b, nullptr, nullptr, EPI_VITQKV, &vr)) return rc;
        } else {
            GemmArgs ga{e->v_xn, C, w.qkv_w, N, 3 * C, C, e->v_qkv, 3 * C, w.qkv_b, nullptr, nullptr, 0, nullptr, 0};
            ga.vrope = VitRope{e->v_cos, e->v_sin, e->v_vt, e->v_vt_stride, C, hd};
            const bool fused = e->v_paired && gemm_fuses_vitqkv(ga);
            SR_TRY(launch_gemm(s, ga, fused ? EPI_VITQKV : EPI_STORE));
            if (!fused) SR_TRY(launch_vit_rope(s, e->v_qkv, N, c.v_heads, hd, e->v_cos, e->v_sin, e->v_vt, e->v_vt_stride, e->v_paired ? 1 : 0));
        }
        const bool full = is_fullatt(c, blk);
        AttnArgs a{e->v_qkv, 3 * C, e->v_qkv + C, 3 * C, hd, e->v_vt, e->v_vt_stride, (long long)hd * e->v_vt_stride,
                   e->v_attn, C, full ? e->v_work_full : e->v_work_win, full ? e->v_nwork_full : e->v_nwork_win,
                   c.v_heads, 1, scale, 0, 64, 0};
        if (!full && e->v_win_all64 && e->v_vt_stride % 4 == 0) a.win64 = 1;     // one wave per (window, head), operands straight into registers
        if (full && e->v_full_aligned) {      // full attention: 128-query blocks that share LDS-DMA-staged tiles (k_attn_prefill2) where it applies
            AttnArgs a2 = a;
            a2.work = e->v_work_full128; a2.n_work = e->v_nwork_full128; a2.q_tile = 128; a2.v2_ok = 1;
            if (attn_prefill_variant(a2, hd) == 2) a = a2;
        }
        SR_TRY(launch_attn_prefill(s, a, hd));
        if (int rc = vit_gemm(e, s, e->v_attn, C, w.proj_w, w.proj_w8, w.proj_s, N, C, C, e->v_x, C, w.proj_b, e->v_x, nullptr, EPI_RESID)) return rc;
        SR_TRY(norm(w.norm2, 1));
        if (int rc = vit_gemm(e, s, xn, C, w.gu_w, w.gu_w8, w.gu_s, N, 2 * e->v_inter_pad, C, e->v_act, e->v_inter_pad, w.gu_b, nullptr, nullptr, EPI_SWIGLU)) return rc;
        if (int rc = vit_gemm(e, s, e->v_act, e->v_inter_pad, w.down_w, w.down_w8, w.down_s, N, C, e->v_inter_pad, e->v_x, C, w.down_b, e->v_x, nullptr, EPI_RESID)) return rc;
    }
    // merger (hf:137-150) with the inverse window permutation fused into the last store (hf:463-465); ln_q normalises rows of C, mlp.0 sees
    // merge^2 of them as one row
    const int unit = c.v_merge * c.v_merge, T = N / unit;
    SR_TRY(norm(e->ln_q, unit));
    if (int rc = vit_gemm(e, s, xn, e->v_mh, e->fc1_w, e->fc1_w8, e->fc1_s, T, e->v_mh, e->v_mh, e->v_m1, e->v_mh, e->fc1_b, nullptr, nullptr, EPI_GELU)) return rc;
    if (int rc = vit_gemm(e, s, e->v_m1, e->v_mh, e->fc2_w, e->fc2_w8, e->fc2_s, T, c.v_out_hidden, e->v_mh, out, c.v_out_hidden, e->fc2_b, nullptr, e->v_rowmap_merge, EPI_STORE)) return rc;
    return 0;
}

int sr_finalize_weights(sr_engine* e, void* stream) {
    enter(e);
    if (!e) return fail(e, -22, "sr_finalize_weights: null engine");
    if (e->finalized) return 0;
    {
        char first[160] = "";
        const int missing = sr_weights_missing(e, first, sizeof first);
        if (missing) return fail(e, -22, "sr_finalize_weights: %d parameters missing, e.g. %s", missing, first);
    }
    hipStream_t s = (hipStream_t)stream;
    if (e->c.lm_weight_dtype >= 1) {
        const int H = e->c.t_hidden, QD = e->c.t_heads * 128;
        // a fused matrix is re-quantised when ALL of its HF tensors were reloaded (a trainer -> engine weight sync sends every
        // parameter); a partial reload would mix fresh bf16 rows with rows that already hold quantised values
        static const unsigned char full[4] = {7, 1, 3, 1};
        for (size_t i = 0; i < e->ll.size(); ++i) {
            LmLayerW& l = e->ll[i];
            for (int m = 0; m < 4; ++m)
                if (l.dirty[m] != 0 && l.dirty[m] != full[m])
                    return fail(e, -22, "fp8 weights: layer %zu matrix %d was only partly reloaded (mask %d of %d)", i, m, l.dirty[m], full[m]);
            if (l.dirty[0]) SR_TRY(launch_quant_f8(s, l.qkv_w, e->t_qn, H, l.qkv_w8, l.qkv_s));
            if (l.dirty[1]) SR_TRY(launch_quant_f8(s, l.o_w, H, QD, l.o_w8, l.o_s));
            if (l.dirty[2]) SR_TRY(launch_quant_f8(s, l.gu_w, 2 * e->t_inter_pad, H, l.gu_w8, l.gu_s));
            if (l.dirty[3]) SR_TRY(launch_quant_f8(s, l.down_w, H, e->t_inter_pad, l.down_w8, l.down_s));
            l.dirty[0] = l.dirty[1] = l.dirty[2] = l.dirty[3] = 0;
        }
        SR_TRY((int)hipStreamSynchronize(s));
    }
    if (e->c.v_weight_dtype == 2) {
        // the bf16 masters stay, so ANY reloaded tensor re-quantises its whole (fused) matrix from them: no partial-reload rule here
        const int C = e->c.v_hidden, IP = e->v_inter_pad;
        for (VitBlockW& b : e->vb) {
            if (b.dirty[0]) SR_TRY(launch_quant_f8_rows(s, b.qkv_w, 3 * C, C, b.qkv_w8, b.qkv_s));
            if (b.dirty[1]) SR_TRY(launch_quant_f8_rows(s, b.proj_w, C, C, b.proj_w8, b.proj_s));
            if (b.dirty[2]) SR_TRY(launch_quant_f8_rows(s, b.gu_w, 2 * IP, C, b.gu_w8, b.gu_s));
            if (b.dirty[3]) SR_TRY(launch_quant_f8_rows(s, b.down_w, C, IP, b.down_w8, b.down_s));
            b.dirty[0] = b.dirty[1] = b.dirty[2] = b.dirty[3] = 0;
        }
        if (e->fc_dirty[0]) SR_TRY(launch_quant_f8_rows(s, e->fc1_w, e->v_mh, e->v_mh, e->fc1_w8, e->fc1_s));
        if (e->fc_dirty[1]) SR_TRY(launch_quant_f8_rows(s, e->fc2_w, e->c.v_out_hidden, e->v_mh, e->fc2_w8, e->fc2_s));
        e->fc_dirty[0] = e->fc_dirty[1] = 0;
        SR_TRY((int)hipStreamSynchronize(s));
    }
    e->finalized = true;
    return 0;
}

// the table entry of a row admitted without parameters of its own: the shared configuration of sr_rows_sampling, keyed by the row
static RowParams default_params(const sr_engine* e) {
    return RowParams{e->rows_temp > 0.f ? 1.0f / e->rows_temp : 0.f, e->rows_topk, e->rows_topp, 1.0f, e->rows_seed, RP_ROW_STREAM};
}

// per-row sampling state, on first use (as the beam state: the workspace and engines that never use it are unchanged).  Every row's entry
// starts as the shared configuration, so that rows admitted before the table existed draw exactly as they did
static int ensure_row_params(sr_engine* e, hipStream_t s) {
    if (e->rp_mem) return 0;
    if (!e->h_rp) SR_TRY((int)hipHostMalloc((void**)&e->h_rp, MAXB * sizeof(RowParams)));
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_rows = take(MAXB * sizeof(RowParams)), o_stage = take(MAXB * sizeof(RowParams)),
                 o_seen = take((size_t)e->n_slots * e->seen_words * sizeof(unsigned));
    void* m = nullptr;
    SR_TRY((int)hipMalloc(&m, off));
    e->rp_rows = reinterpret_cast<RowParams*>(static_cast<char*>(m) + o_rows);
    e->rp_stage = reinterpret_cast<RowParams*>(static_cast<char*>(m) + o_stage);
    e->rp_seen = reinterpret_cast<unsigned*>(static_cast<char*>(m) + o_seen);
    for (int i = 0; i < MAXB; ++i) e->h_rp[i] = default_params(e);
    hipError_t r = hipMemcpyAsync(e->rp_rows, e->h_rp, MAXB * sizeof(RowParams), hipMemcpyHostToDevice, s);
    if (r == hipSuccess) r = hipMemsetAsync(e->rp_seen, 0, (size_t)e->n_slots * e->seen_words * sizeof(unsigned), s);
    if (r == hipSuccess) r = hipStreamSynchronize(s);
    if (r != hipSuccess) { (void)hipFree(m); return (int)r; }
    e->rp_mem = m;
    return 0;
}

// installs the staged admission's sequences into batch rows (row state + pending first token); runs on the DECODE stream, between steps
static int commit_admission(sr_engine* e, const int32_t* rows, int n, hipStream_t s) {
    const sr_config& c = e->c;
    // the staged sequences may be committed in several portions (rows free up one by one): `off` = how many are installed already
    const int off = e->staged_off;
    for (int i = 0; i < n; ++i) e->h_rows[off + i] = rows[i];
    SR_TRY((int)hipMemcpyAsync(e->d_adm + off, e->h_rows + off, (size_t)n * 4, hipMemcpyHostToDevice, s));
    const int MB = c.max_batch;
    AdmitArgs aa{e->d_adm + off, e->d_adm + MAXB + off, e->d_adm + 2 * MAXB + off, e->d_adm + 3 * MAXB + off, e->d_adm + 4 * MAXB + off, n,
                 e->d_ctx_len, e->d_pos, e->d_slots, e->d_finished, e->d_step, e->d_row_limit, e->d_ngen,
                 e->d_amax_val, e->d_amax_idx, gemv_f32_blocks(c.t_vocab, MB, c.t_hidden, fused_norms(e, MB) ? 1 : 0), e->d_adm_slots + off};
    if (e->staged_rp) {              // per-row table: the first tokens drawn under the staged entries, and the entries, go to the rows
        aa.first_pick = e->d_adm_pick + off; aa.sampled = e->d_sampled;
        aa.stage_params = e->rp_stage + off; aa.row_params = e->rp_rows;
    } else if (e->rp_mem) {          // staged before the table existed: the shared entry, and the greedy first token where the per-row graph reads it
        aa.row_params = e->rp_rows; aa.dflt = default_params(e);
        if (!(e->rows_temp > 0.f)) aa.sampled = e->d_sampled;
    }
    SR_TRY(launch_admit_rows(s, aa));
    // the rows' logs: the staged position-0 records (when the admission recorded), the rest cleared.  Also with the switch off, once a log
    // exists: the switch may go on again in the middle of this occupant's run, and its earlier positions must not show the previous one's records
    if (e->lp_mem) {
        const bool rec = e->staged_lp;
        LogprobAdmitArgs la{e->d_adm + off, n, c.max_new_tokens, rec ? e->lps_lp + off : nullptr, e->lps_ids + (size_t)off * LP_MAXN,
                            e->lps_tlp + (size_t)off * LP_MAXN, e->lp_log, e->lp_ids, e->lp_tlp};
        SR_TRY(launch_logprob_admit(s, la));
    }
    if (e->rows_temp > 0.f && !e->staged_rp) SR_TRY(launch_scatter_rows(s, e->d_adm + off, e->d_adm_pick + off, e->d_sampled, n));   // the drawn first tokens
    e->staged_n -= n;
    e->staged_off = e->staged_n ? off + n : 0;
    return 0;
}

// the packed prompts as every prefill entry point receives them
struct Prompts {
    const int64_t *ids, *pos3; const int32_t* seq_lens; int B;
    const void* image_embeds; int n_image_rows;
    float* logits_out;                      // optional: float32 [B, V] of the last positions
    void* stream;
};
struct PrefillArgs {
    Prompts p;
    const int32_t* slots = nullptr;         // the KV slot prompt b is prefilled into
    float* all_logits_out = nullptr;        // static only (sr_forward_logits): float32 logits of every position
    // `admission`: into the continuous batch (row state untouched until the commit, admission-owned scratch) instead of a static batch
    // that (re)initialises rows 0..B-1.  The fields below are read for an admission only
    bool admission = false;
    const int32_t* limits = nullptr;        // max_new per prompt
    bool commit = false;                    // install the rows right away (rows = slots: the plain sr_admit); false = stage, sr_admit_commit installs later
    // `fanout` / `fork_slots` (both null: one sequence per prompt): prompt b becomes fanout[b] staged sequences (prompt-major) whose
    // KV slots are fork_slots (sum of fanout entries); it is prefilled once into slots[b] (= its first fork's slot), its LM head runs once, and
    // one k_kv_fanout launch copies every prompt's prefix into the slots of its other forks.  Each staged sequence draws its own first token.
    const int32_t *fanout = nullptr, *fork_slots = nullptr;
    const sr_sampling* sampling = nullptr;  // optional: one entry per staged sequence (the per-row table exists: ensure_row_params)
};

static int prefill_impl(sr_engine* e, const PrefillArgs& pa) {
    enter(e);
    const auto& [ids, pos3, seq_lens, B, image_embeds, n_image_rows, logits_out, stream] = pa.p;
    const int32_t* slots = pa.slots;
    const bool admission = pa.admission;
    const sr_sampling* smp = pa.sampling;
    if (!e || !ids || !pos3 || !seq_lens || !slots) return fail(e, -22, "sr_prefill: null argument");
    char miss[160];
    if (sr_weights_missing(e, miss, sizeof miss)) return fail(e, -61, "weights missing, e.g. '%s'", miss);
    const sr_config& c = e->c;
    if (c.lm_weight_dtype >= 1 && !e->finalized) return fail(e, -22, "fp8 weights: call sr_finalize_weights after loading");
    if (B < 1 || B > c.max_batch) return fail(e, -22, "sr_prefill: B=%d outside 1..%d", B, c.max_batch);
    hipStream_t s = (hipStream_t)stream;
    int n_tok = 0;
    for (int b = 0; b < B; ++b) {
        if (seq_lens[b] < 1 || seq_lens[b] + 1 > c.max_ctx)
            return fail(e, -22, "sequence %d length %d does not fit max_ctx %d", b, seq_lens[b], c.max_ctx);
        if (slots[b] < 0 || slots[b] >= e->n_slots) return fail(e, -22, "KV slot %d out of range 0..%d", slots[b], e->n_slots - 1);
        n_tok += seq_lens[b];
    }
    if (n_tok > c.max_prefill_tokens) return fail(e, -22, "%d prompt tokens exceed max_prefill_tokens %d", n_tok, c.max_prefill_tokens);

    // ---- control arrays (host) -> device
    SR_TRY(stage_begin(e));
    int* h_src = reinterpret_cast<int*>(e->h_stage);
    int* h_pos = h_src + n_tok;
    int* h_slot = h_pos + 3 * n_tok;
    int* h_idx = h_slot + n_tok;
    int* h_last = h_idx + n_tok;
    int* h_state = h_last + MAXB;           // [ctx_len | pos | slots | limit] x MAXB, per staged sequence
    for (int i = 0; i < 4 * MAXB; ++i) h_state[i] = 0;
    int* h_map = h_state + 4 * MAXB;        // fan-out (d_fan): prompt of each staged sequence, then [src slot | L | first fork index | forks - 1] per group
    int* h_grp = h_map + MAXB;
    AttnWork* h_work = reinterpret_cast<AttnWork*>(((uintptr_t)(h_grp + 4 * MAXB) + 15) & ~(uintptr_t)15);
    int n_work = 0, img_row = 0, t0 = 0, n_seq = 0, n_groups = 0, max_L = 0;
    const int KVH = c.t_kv_heads;
    for (int b = 0; b < B; ++b) {
        const int S = seq_lens[b];
        long long maxpos = 0;
        for (int i = 0; i < S; ++i) {
            const int t = t0 + i;
            const int64_t id = ids[t];
            if (id < 0 || id >= c.t_vocab) return fail(e, -22, "token id %lld out of range", (long long)id);
            // image placeholders consume the image feature rows in order (hf:1210-1216 masked_scatter)
            h_src[t] = (image_embeds && id == c.image_token_id) ? -(img_row++) - 1 : (int)id;
            for (int a = 0; a < 3; ++a) {
                const int64_t p = pos3[(size_t)a * n_tok + t];
                h_pos[(size_t)a * n_tok + t] = (int)p;
                if (p < 0 || p > c.max_ctx) return fail(e, -22, "position id %lld outside 0..max_ctx (%d)", (long long)p, c.max_ctx);
                if (p > maxpos) maxpos = p;
            }
            h_slot[t] = slots[b];
            h_idx[t] = i;
        }
        if (!admission) { e->pre_len[b] = S; e->pre_slot[b] = slots[b]; e->pre_pos[b] = (int)maxpos; }
        for (int q0 = 0; q0 < S; q0 += 64)
            h_work[n_work++] = AttnWork{t0 + q0, S, q0, slots[b] * KVH * c.max_ctx, (long long)slots[b] * KVH * 128 * c.max_ctx};
        h_last[b] = t0 + S - 1;
        const int f = pa.fanout ? pa.fanout[b] : 1;
        if (f > 1) {
            int* g = h_grp + 4 * n_groups++;
            g[0] = slots[b]; g[1] = S; g[2] = n_seq + 1; g[3] = f - 1;
            max_L = std::max(max_L, S);
        }
        for (int j = 0; j < f; ++j, ++n_seq) {
            h_map[n_seq] = b;
            h_state[n_seq] = S;                     // keys in the cache; k_step_advance adds the new token before each forward
            h_state[MAXB + n_seq] = (int)maxpos;      // decode positions continue at max+1 on all three axes
                                                    // (reference rule: roll/utils/functionals.py:816-818)
            h_state[2 * MAXB + n_seq] = pa.fork_slots ? pa.fork_slots[n_seq] : slots[b];
            h_state[3 * MAXB + n_seq] = admission ? pa.limits[b] : 0x7f7f7f7f;
        }
        t0 += S;
    }
    if (image_embeds && img_row != n_image_rows)
        return fail(e, -22, "image features and image tokens do not match: %d tokens, %d feature rows", img_row, n_image_rows);
    const size_t total = reinterpret_cast<char*>(h_work + n_work) - e->h_stage;
    if (total > e->stage_bytes) return fail(e, -12, "control staging too small");
    // once the per-row table exists, every admission stages its sequences' entries (its own, or the shared configuration restated)
    // (h_rp is free again: stage_begin waited for the event recorded behind the previous upload, which follows this copy on its stream)
    const bool rp_stage = admission && e->rp_mem;
    if (rp_stage) {
        for (int i = 0; i < n_seq; ++i) {
            RowParams p = default_params(e);
            if (smp) p = RowParams{smp[i].temperature > 0.f ? 1.0f / smp[i].temperature : 0.f, smp[i].top_k, smp[i].top_p, smp[i].repetition_penalty,
                                   smp[i].seed, smp[i].stream < 0 ? RP_ROW_STREAM : (unsigned)smp[i].stream};
            e->h_rp[i] = p;
        }
        SR_TRY((int)hipMemcpyAsync(e->rp_stage, e->h_rp, (size_t)n_seq * sizeof(RowParams), hipMemcpyHostToDevice, s));
    }
    SR_TRY(stage_upload(e, 0, total, s));
    auto dmirror = [&](const void* hptr) { return e->d_stage + (reinterpret_cast<const char*>(hptr) - e->h_stage); };
    SR_TRY((int)hipMemcpyAsync(e->t_src, dmirror(h_src), (size_t)n_tok * 4, hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->t_pos3, dmirror(h_pos), (size_t)n_tok * 12, hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->t_slot, dmirror(h_slot), (size_t)n_tok * 4, hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->t_idx, dmirror(h_idx), (size_t)n_tok * 4, hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->t_lastrow, dmirror(h_last), MAXB * 4, hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->t_work, dmirror(h_work), n_work * sizeof(AttnWork), hipMemcpyDeviceToDevice, s));
    if (!admission) {       // static batch: rows 0..B-1 are (re)initialised, all other rows are dropped
        SR_TRY((int)hipMemcpyAsync(e->d_ctx_len, dmirror(h_state), MAXB * 4, hipMemcpyDeviceToDevice, s));
        SR_TRY((int)hipMemcpyAsync(e->d_pos, dmirror(h_state + MAXB), MAXB * 4, hipMemcpyDeviceToDevice, s));
        SR_TRY((int)hipMemcpyAsync(e->d_slots, dmirror(h_state + 2 * MAXB), MAXB * 4, hipMemcpyDeviceToDevice, s));
        SR_TRY((int)hipMemsetAsync(e->d_finished, 0, MAXB * 4, s));
        SR_TRY((int)hipMemsetAsync(e->d_step, 0, MAXB * 4, s));
        SR_TRY((int)hipMemsetAsync(e->d_row_limit, 0x7f, MAXB * 4, s));
        SR_TRY((int)hipMemsetAsync(e->d_ngen, 0, MAXB * 4, s));
    } else {             // admission: [rows | ctx | pos | limit] for the new rows only; installed after the LM head below
        SR_TRY((int)hipMemcpyAsync(e->d_adm_slots, dmirror(h_state + 2 * MAXB), MAXB * 4, hipMemcpyDeviceToDevice, s));
        SR_TRY((int)hipMemcpyAsync(e->d_adm + MAXB, dmirror(h_state), MAXB * 4, hipMemcpyDeviceToDevice, s));
        SR_TRY((int)hipMemcpyAsync(e->d_adm + 2 * MAXB, dmirror(h_state + MAXB), MAXB * 4, hipMemcpyDeviceToDevice, s));
        SR_TRY((int)hipMemcpyAsync(e->d_adm + 3 * MAXB, dmirror(h_state + 3 * MAXB), MAXB * 4, hipMemcpyDeviceToDevice, s));
        if (n_groups) SR_TRY((int)hipMemcpyAsync(e->d_fan, dmirror(h_map), 5 * MAXB * 4, hipMemcpyDeviceToDevice, s));
    }

    // ---- forward over the packed tokens
    const int H = c.t_hidden, QD = c.t_heads * 128;
    SR_TRY(launch_embed(s, e->t_src, e->embed, static_cast<const bf16_t*>(image_embeds), e->t_x, n_tok, H, 1));
    const float scale = (float)(1.0 / sqrt(128.0));
    const bool splitk = !admission && prefill_splitk(e, n_tok);
    bool pending = false;        // split-K: the down-projection's slabs have not been added to t_x yet
    for (int l = 0; l < c.t_layers; ++l) {
        const LmLayerW& w = e->ll[l];
        bf16_t* kc = e->kcache + (size_t)l * e->kv_layer_elems;
        bf16_t* vc = e->vtcache + (size_t)l * e->kv_layer_elems;
        if (pending) SR_TRY(launch_resid_rmsnorm(s, e->t_x, e->t_slabs, SPLITK_KS, w.ln1, e->t_xn, n_tok, H, c.t_rms_eps, 0, 1));
        else SR_TRY(launch_rmsnorm(s, e->t_x, w.ln1, e->t_xn, n_tok, H, c.t_rms_eps, 0, 1));
        // q/k/v Linear; mRoPE and the KV-cache write ride in the GEMM epilogue when the 256-tile kernel takes the shape (large batches),
        // otherwise they are the separate launch of round 1 (bit-identical results either way)
        const QkvRope qr{e->t_pos3, e->t_slot, e->t_idx, e->rope_cos, e->rope_sin, kc, vc, n_tok, c.t_heads, c.t_kv_heads,
                         c.mrope_section[0], c.mrope_section[0] + c.mrope_section[1], c.max_ctx};
        bool fused_qkv = false;
        if (int rc = lm_gemm(e, s, e->t_xn, H, w.qkv_w, w.qkv_w8, w.qkv_s, n_tok, e->t_qn, H, e->t_qkv, e->t_qn, w.qkv_b, nullptr, EPI_STORE, &qr, &fused_qkv)) return rc;
        if (!fused_qkv) {
            LmRopeArgs ra{e->t_qkv, n_tok, c.t_heads, c.t_kv_heads, e->t_pos3, e->t_slot, e->t_idx, e->rope_cos, e->rope_sin,
                          c.mrope_section[0], c.mrope_section[0] + c.mrope_section[1], kc, vc, c.max_ctx};
            SR_TRY(launch_lm_rope_prefill(s, ra));
        }
        AttnArgs a{e->t_qkv, e->t_qn, kc, 128, (long long)c.max_ctx * 128, vc, c.max_ctx, (long long)128 * c.max_ctx,
                   e->t_attn, QD, e->t_work, n_work, c.t_heads, e->t_group, scale, 1, 64, 1};      // max_ctx % 64 == 0: aligned, readable key runs
        SR_TRY(launch_attn_prefill(s, a, 128));
        if (splitk) {
            if (int rc = lm_gemm(e, s, e->t_attn, QD, w.o_w, w.o_w8, w.o_s, n_tok, H, QD, e->t_slabs, H, nullptr, nullptr, EPI_F32, nullptr, nullptr, SPLITK_KS)) return rc;
            SR_TRY(launch_resid_rmsnorm(s, e->t_x, e->t_slabs, SPLITK_KS, w.ln2, e->t_xn, n_tok, H, c.t_rms_eps, 0, 1));
        } else {
            if (int rc = lm_gemm(e, s, e->t_attn, QD, w.o_w, w.o_w8, w.o_s, n_tok, H, QD, e->t_x, H, nullptr, e->t_x, EPI_RESID)) return rc;
            SR_TRY(launch_rmsnorm(s, e->t_x, w.ln2, e->t_xn, n_tok, H, c.t_rms_eps, 0, 1));
        }
        if (int rc = lm_gemm(e, s, e->t_xn, H, w.gu_w, w.gu_w8, w.gu_s, n_tok, 2 * e->t_inter_pad, H, e->t_act, e->t_inter_pad, nullptr, nullptr, EPI_SWIGLU)) return rc;
        if (splitk) {
            if (int rc = lm_gemm(e, s, e->t_act, e->t_inter_pad, w.down_w, w.down_w8, w.down_s, n_tok, H, e->t_inter_pad, e->t_slabs, H, nullptr, nullptr, EPI_F32, nullptr, nullptr, SPLITK_KS)) return rc;
            pending = true;
        } else if (int rc = lm_gemm(e, s, e->t_act, e->t_inter_pad, w.down_w, w.down_w8, w.down_s, n_tok, H, e->t_inter_pad, e->t_x, H, nullptr, e->t_x, EPI_RESID)) return rc;
    }
    // last position of every sequence -> final norm -> tied LM head (hf:1386-1387) -> greedy token
    // (split-K: the last down-projection's slabs still have to reach t_x; the norm output is only used by the all-positions path)
    if (pending) SR_TRY(launch_resid_rmsnorm(s, e->t_x, e->t_slabs, SPLITK_KS, e->final_norm, e->t_xn, n_tok, H, c.t_rms_eps, 0, 1));
    if (pa.all_logits_out) {       // every position: final norm over all rows, tied LM head as an MFMA GEMM with float32 output
        if (!pending) SR_TRY(launch_rmsnorm(s, e->t_x, e->final_norm, e->t_xn, n_tok, H, c.t_rms_eps, 0, 1));
        if (int rc = gemm(e, s, e->t_xn, H, e->embed, n_tok, c.t_vocab, H, pa.all_logits_out, c.t_vocab, nullptr, nullptr, nullptr, EPI_F32, 1)) return rc;
    }
    // (an admission keeps to scratch of its own -- d_xadm / d_xadm_n, the *_adm logits and partials -- because it may run on another
    // stream while the rows decode)
    bf16_t* xl = admission ? e->d_xadm : e->d_xa;
    SR_TRY(launch_gather_rows(s, e->t_x, e->t_lastrow, xl, B, H));
    if (!admission) {
        if (int rc = enqueue_lm_head(e, B, xl, e->d_xb, false, s)) return rc;
        if (logits_out) SR_TRY((int)hipMemcpyAsync(logits_out, e->d_logits, (size_t)B * c.t_vocab * 4, hipMemcpyDeviceToDevice, s));
        e->h_ctx_hi = 0;
        for (int b = 0; b < B; ++b) e->h_ctx_hi = std::max(e->h_ctx_hi, (int)seq_lens[b]);
        e->prefilled_B = B;
        e->rows_mode = false;
        return 0;
    }
    // admission: final norm + LM head into the admission scratch, greedy first token, then install the rows.  ONE kernel path whatever the
    // number of sequences admitted together (block-per-row norm, 32-row MFMA GEMV -- what a static batch of more than 16 runs), so that a
    // request's first token does not depend on how the scheduler grouped it
    {
        GemvArgs g = gv(xl, H, e->embed, B, c.t_vocab, H, e->d_logits_adm, c.t_vocab);
        g.amax_val = e->d_amax_val_adm; g.amax_idx = e->d_amax_idx_adm;
        const int xt = x_tiled_ok(e) ? 1 : 0;
        SR_TRY(launch_rmsnorm(s, xl, e->final_norm, e->d_xadm_n, B, H, c.t_rms_eps, xt));
        g.x = e->d_xadm_n; g.x_tiled = xt; g.force32 = 1;
        SR_TRY(launch_gemv(s, g, GV_F32));
    }
    if (logits_out) SR_TRY((int)hipMemcpyAsync(logits_out, e->d_logits_adm, (size_t)B * c.t_vocab * 4, hipMemcpyDeviceToDevice, s));
    // first token of every staged sequence: the forks of a prompt read its logits row (row map), each draws at its own staged index
    const int* row_map = n_groups ? e->d_fan : nullptr;
    SR_TRY(launch_argmax(s, e->d_logits_adm, n_seq, c.t_vocab, e->d_adm + 4 * MAXB, row_map));
    if (rp_stage) {                // per-row table: each staged sequence's slot bitmap = its prompt, then its first token under its own entry
        SR_TRY(launch_mark_staged(s, e->t_src, e->t_lastrow, n_groups ? e->d_fan : nullptr, e->d_adm_slots, e->rp_seen, e->seen_words, n_seq));
        // (salt: the shared path's seed of this admission for the entries keyed by the row -- sr_rows_sampling's draw below, restated)
        SampleArgs sa = sample_args(e, n_seq, true);
        sa.row_map = row_map;
        sa.seen = e->rp_seen; sa.params = e->rp_stage; sa.seen_slot = e->d_adm_slots;
        sa.seed = e->rows_temp > 0.f ? 0x9E3779B9u * ++e->adm_count : 0u;
        SR_TRY(launch_sample(s, sa));
    } else if (e->rows_temp > 0.f) {      // sampling mode: the first token of the new rows is drawn from the admission logits
        SampleArgs sa = sample_args(e, n_seq, true);
        sa.row_map = row_map;
        sa.inv_temp = 1.0f / e->rows_temp; sa.top_k = e->rows_topk; sa.top_p = e->rows_topp;
        sa.seed = e->rows_seed ^ (0x9E3779B9u * ++e->adm_count);
        SR_TRY(launch_sample(s, sa));
    }
    e->staged_lp = e->lp_n >= 0;
    if (e->staged_lp) {            // position-0 records of the staged sequences (a fork reads its prompt's row), carried until the commit
        const bool drawn = rp_stage || e->rows_temp > 0.f;
        LogprobArgs la{e->d_logits_adm, c.t_vocab, c.t_vocab, n_seq, e->lp_n, row_map, e->lp_part_adm, drawn ? e->d_adm_pick : nullptr, nullptr, nullptr, 0,
                       e->lps_lp, nullptr, e->lps_ids, e->lps_tlp};
        SR_TRY(launch_logprobs(s, la));
    }
    if (n_groups) {                // the prompts' KV prefixes into the slots of their other forks (d_adm_slots holds every fork's slot in staged order)
        KvFanoutArgs fa{e->kcache, e->vtcache, (long long)e->kv_layer_elems, c.t_layers, c.t_kv_heads, c.max_ctx, e->d_adm_slots, 0, 0, 0,
                        e->d_fan + MAXB, n_groups, max_L};
        SR_TRY(launch_kv_fanout(s, fa));
    }
    e->staged_n = n_seq;
    e->staged_off = 0;
    e->staged_rp = rp_stage;
    if (pa.commit) return commit_admission(e, pa.fork_slots ? pa.fork_slots : slots, n_seq, s);
    return 0;
}

int sr_prefill(sr_engine* e, const int64_t* ids, const int64_t* pos3, const int32_t* seq_lens, const int32_t* slots, int B,
               const void* image_embeds, int n_image_rows, float* logits_out, void* stream) {
    PrefillArgs pa;
    pa.p = Prompts{ids, pos3, seq_lens, B, image_embeds, n_image_rows, logits_out, stream};
    pa.slots = slots;
    return prefill_impl(e, pa);
}

int sr_forward_logits(sr_engine* e, const int64_t* ids, const int64_t* pos3, const int32_t* seq_lens, int B, const void* image_embeds,
                      int n_image_rows, float* all_logits_out, void* stream) {
    if (!all_logits_out) return fail(e, -22, "sr_forward_logits: null output");
    if (!e || B < 1 || B > MAXB) return fail(e, -22, "sr_forward_logits: bad batch");
    int32_t slots[MAXB];
    for (int b = 0; b < B; ++b) slots[b] = b;
    PrefillArgs pa;
    pa.p = Prompts{ids, pos3, seq_lens, B, image_embeds, n_image_rows, /*logits_out*/ nullptr, stream};
    pa.slots = slots;
    pa.all_logits_out = all_logits_out;
    return prefill_impl(e, pa);
}

// ---- continuous batching: batch rows with independent lifecycles (row index = KV slot); a decode step always runs all
// max_batch rows, rows that are free or finished are masked by their `finished` flag
int sr_rows_begin(sr_engine* e, void* stream) {
    enter(e);
    if (!e) return fail(e, -22, "sr_rows_begin: null engine");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> st(5 * MAXB, 0);
    for (int i = 0; i < MAXB; ++i) { st[i] = 1; st[2 * MAXB + i] = 1; st[3 * MAXB + i] = 0; st[4 * MAXB + i] = i; }   // ctx 1 | pos 0 | finished 1 | step 0 | slots
    SR_TRY((int)hipMemcpyAsync(e->d_ctx_len, st.data(), MAXB * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->d_pos, st.data() + MAXB, MAXB * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->d_finished, st.data() + 2 * MAXB, MAXB * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->d_step, st.data() + 3 * MAXB, MAXB * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->d_slots, st.data() + 4 * MAXB, MAXB * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemsetAsync(e->d_row_limit, 0, MAXB * 4, s));
    SR_TRY((int)hipMemsetAsync(e->d_ngen, 0, MAXB * 4, s));
    if (e->lp_mem) SR_TRY(launch_logprob_clear(s, e->c.max_batch * e->c.max_new_tokens, e->lp_log, e->lp_ids, e->lp_tlp));
    SR_TRY((int)hipStreamSynchronize(s));
    e->staged_lp = false;
    e->rows_mode = true;
    e->staged_n = e->staged_off = 0;
    e->prefilled_B = e->c.max_batch;
    e->h_ctx_hi = 0;
    e->rows_temp = 0.f;
    e->rows_perrow = e->staged_rp = false;
    return 0;
}

int sr_rows_per_row(sr_engine* e, int on, void* stream) {
    enter(e);
    if (!e || !e->rows_mode) return fail(e, -22, "sr_rows_per_row: call sr_rows_begin first");
    hipStream_t s = (hipStream_t)stream;
    if (!on) { e->rows_perrow = false; return 0; }
    SR_TRY(ensure_row_params(e, s));
    if (!e->rows_perrow && !(e->rows_temp > 0.f)) {
        // greedy rows keep their pending token in the LM-head partials (k_step reduces them); the per-row graph reads d_sampled
        const int MB = e->c.max_batch;
        SR_TRY(launch_next_ids(s, e->d_amax_val, e->d_amax_idx, gemv_f32_blocks(e->c.t_vocab, MB, e->c.t_hidden, fused_norms(e, MB) ? 1 : 0), MB,
                               e->d_sampled));
    }
    e->rows_perrow = true;
    return 0;
}

// refuses a bad entry by name; -> 0 or the error code
static int check_sampling(sr_engine* e, const char* fn, const sr_sampling* p, int n) {
    for (int i = 0; i < n; ++i) {
        if (!(p[i].temperature >= 0.f)) return fail(e, -22, "%s: sequence %d: temperature %g < 0", fn, i, (double)p[i].temperature);
        if (p[i].top_k > 1024) return fail(e, -22, "%s: sequence %d: top_k %d > 1024", fn, i, p[i].top_k);
        if (!(p[i].top_p > 0.f && p[i].top_p <= 1.f)) return fail(e, -22, "%s: sequence %d: top_p %g outside (0, 1]", fn, i, (double)p[i].top_p);
        if (!(p[i].repetition_penalty > 0.f))
            return fail(e, -22, "%s: sequence %d: repetition_penalty %g <= 0", fn, i, (double)p[i].repetition_penalty);
    }
    return 0;
}

int sr_rows_sampling(sr_engine* e, float temperature, int top_k, float top_p, uint32_t seed) {
    if (!e || !e->rows_mode) return fail(e, -22, "sr_rows_sampling: call sr_rows_begin first");
    if (temperature > 0.f && (top_k > 1024 || !(top_p > 0.f) || top_p > 1.f))
        return fail(e, -22, "sr_rows_sampling: top_k <= 1024 (<= 0: no top-k bound) and 0 < top_p <= 1 required");
    e->rows_temp = temperature > 0.f ? temperature : 0.f;
    e->rows_topk = top_k; e->rows_topp = top_p; e->rows_seed = seed; e->adm_count = 0;
    return 0;
}

// checks of a fan-out admission (sr_admit_fanout / sr_admit_stage_fanout and their all-ones forms): n prompts, fanout[i] >= 1 sequences each,
// sum <= MAXB (the staging capacity), every sequence's KV slot (or row) distinct and in range; -> the sum, or a negative error
static int check_fanout(sr_engine* e, const char* fn, const int32_t* seq_lens, const int32_t* fanout, const int32_t* dst, int n, int dst_hi,
                        const char* what, const int32_t* max_new) {
    if (!e->rows_mode) return fail(e, -22, "%s: call sr_rows_begin first", fn);
    if (e->staged_n) return fail(e, -22, "%s: %d staged sequences are waiting for sr_admit_commit", fn, e->staged_n);
    if (n < 1 || n > e->c.max_batch) return fail(e, -22, "%s: %d prompts outside 1..%d", fn, n, e->c.max_batch);
    int total = 0;
    for (int i = 0; i < n; ++i) {
        if (max_new[i] < 1 || max_new[i] > e->c.max_new_tokens || seq_lens[i] + max_new[i] > e->c.max_ctx)
            return fail(e, -22, "%s: sequence %d (len %d, max_new %d) does not fit max_new_tokens %d / max_ctx %d", fn, i, seq_lens[i],
                        max_new[i], e->c.max_new_tokens, e->c.max_ctx);
        const int f = fanout ? fanout[i] : 1;
        if (f < 1) return fail(e, -22, "%s: fanout %d of prompt %d is below 1", fn, f, i);
        total += f;
        if (total > MAXB) return fail(e, -22, "%s: %d forked sequences exceed the staging capacity %d (MAXB)", fn, total, MAXB);
    }
    for (int i = 0; i < total; ++i) {
        if (dst[i] < 0 || dst[i] >= dst_hi) return fail(e, -22, "%s: %s %d out of range 0..%d", fn, what, dst[i], dst_hi - 1);
        for (int j = 0; j < i; ++j)
            if (dst[i] == dst[j]) return fail(e, -22, "%s: %s %d given twice", fn, what, dst[i]);
    }
    return total;
}

// the KV slot each prompt is prefilled into: its first fork's
static void first_forks(const int32_t* fanout, const int32_t* dst, int n, int32_t* out) {
    for (int i = 0, k = 0; i < n; k += fanout ? fanout[i] : 1, ++i) out[i] = dst[k];
}

// Every admission entry point: `fn` names it in refusals; `dst` = one destination per staged sequence, prompt-major: batch rows
// (installed right away, row r uses KV slot r) or spare KV slots (staged: sr_admit_commit installs later).  `sampling` comes from the
// *_sampling entries only: they create the per-row table on first use, after which EVERY admission stages table entries
enum AdmitTo { TO_ROWS, TO_SPARE_SLOTS };
static int admit(sr_engine* e, const char* fn, AdmitTo to, const Prompts& p, const int32_t* fanout, const int32_t* dst, const int32_t* max_new,
                 const sr_sampling* sampling) {
    enter(e);
    if (!e || !dst || !max_new || !p.seq_lens) return fail(e, -22, "%s: null argument", fn);
    const bool rows = to == TO_ROWS;
    const int total = check_fanout(e, fn, p.seq_lens, fanout, dst, p.B, rows ? e->c.max_batch : e->n_slots, rows ? "row" : "KV slot", max_new);
    if (total < 0) return total;
    if (sampling) {
        if (int rc = check_sampling(e, fn, sampling, total)) return rc;
        SR_TRY(ensure_row_params(e, (hipStream_t)p.stream));
    }
    int32_t first[MAXB];
    first_forks(fanout, dst, p.B, first);
    PrefillArgs pa;
    pa.p = p;
    pa.slots = first;
    pa.admission = true; pa.limits = max_new; pa.commit = rows;
    pa.fanout = fanout; pa.fork_slots = dst; pa.sampling = sampling;
    return prefill_impl(e, pa);
}

// (sr_admit_fanout and sr_admit_stage_fanout report themselves under the names of their all-ones forms)
int sr_admit_fanout(sr_engine* e, const int64_t* ids, const int64_t* pos3, const int32_t* seq_lens, const int32_t* fanout, const int32_t* rows,
                    const int32_t* max_new, int n, const void* image_embeds, int n_image_rows, float* logits_out, void* stream) {
    return admit(e, "sr_admit", TO_ROWS, Prompts{ids, pos3, seq_lens, n, image_embeds, n_image_rows, logits_out, stream}, fanout, rows, max_new, nullptr);
}

int sr_admit(sr_engine* e, const int64_t* ids, const int64_t* pos3, const int32_t* seq_lens, const int32_t* rows, const int32_t* max_new,
             int n, const void* image_embeds, int n_image_rows, float* logits_out, void* stream) {
    return sr_admit_fanout(e, ids, pos3, seq_lens, nullptr, rows, max_new, n, image_embeds, n_image_rows, logits_out, stream);
}

// Admission in two halves, so that the expensive half can run UNDER the decode steps of the running rows on another (CU-masked)
// stream: sr_admit_stage = ViT-fed prefill of n sequences into SPARE KV slots + LM head + first-token choice (touches no row state and
// only admission-owned scratch); sr_admit_commit = install them into free batch rows (row -> KV slot indirection), on the decode
// stream, between two steps, once the staging stream's work is known to be complete (the caller orders the streams with an event).
int sr_admit_stage_fanout(sr_engine* e, const int64_t* ids, const int64_t* pos3, const int32_t* seq_lens, const int32_t* fanout,
                          const int32_t* kv_slots, const int32_t* max_new, int n, const void* image_embeds, int n_image_rows, float* logits_out,
                          void* stream) {
    return admit(e, "sr_admit_stage", TO_SPARE_SLOTS, Prompts{ids, pos3, seq_lens, n, image_embeds, n_image_rows, logits_out, stream}, fanout, kv_slots, max_new,
                 nullptr);
}

int sr_admit_stage(sr_engine* e, const int64_t* ids, const int64_t* pos3, const int32_t* seq_lens, const int32_t* kv_slots, const int32_t* max_new,
                   int n, const void* image_embeds, int n_image_rows, float* logits_out, void* stream) {
    return sr_admit_stage_fanout(e, ids, pos3, seq_lens, nullptr, kv_slots, max_new, n, image_embeds, n_image_rows, logits_out, stream);
}

int sr_admit_stage_sampling(sr_engine* e, const int64_t* ids, const int64_t* pos3, const int32_t* seq_lens, const int32_t* fanout,
                            const int32_t* kv_slots, const int32_t* max_new, const sr_sampling* sampling, int n, const void* image_embeds,
                            int n_image_rows, float* logits_out, void* stream) {
    if (!sampling) return fail(e, -22, "sr_admit_stage_sampling: null argument");
    return admit(e, "sr_admit_stage_sampling", TO_SPARE_SLOTS, Prompts{ids, pos3, seq_lens, n, image_embeds, n_image_rows, logits_out, stream}, fanout, kv_slots,
                 max_new, sampling);
}

int sr_admit_sampling(sr_engine* e, const int64_t* ids, const int64_t* pos3, const int32_t* seq_lens, const int32_t* fanout, const int32_t* rows,
                      const int32_t* max_new, const sr_sampling* sampling, int n, const void* image_embeds, int n_image_rows, float* logits_out,
                      void* stream) {
    if (!sampling) return fail(e, -22, "sr_admit_sampling: null argument");
    return admit(e, "sr_admit_sampling", TO_ROWS, Prompts{ids, pos3, seq_lens, n, image_embeds, n_image_rows, logits_out, stream}, fanout, rows, max_new, sampling);
}

int sr_admit_commit(sr_engine* e, const int32_t* rows, int n, void* stream) {
    enter(e);
    if (!e || !rows) return fail(e, -22, "sr_admit_commit: null argument");
    if (!e->rows_mode || n > e->staged_n || n < 1) return fail(e, -22, "sr_admit_commit: %d rows given, %d sequences staged", n, e ? e->staged_n : 0);
    for (int i = 0; i < n; ++i) {
        if (rows[i] < 0 || rows[i] >= e->c.max_batch) return fail(e, -22, "sr_admit_commit: row %d out of range", rows[i]);
        for (int j = 0; j < i; ++j)
            if (rows[i] == rows[j]) return fail(e, -22, "sr_admit_commit: row %d given twice", rows[i]);
    }
    return commit_admission(e, rows, n, (hipStream_t)stream);
}

int sr_decode(sr_engine* e, const int32_t* host_slots, int B, int max_new, const int32_t* host_eos, int n_eos, int32_t pad_id,
              int32_t* tokens_out, float* logits_trace, const int32_t* forced, int use_graph, void* stream, int* steps_done) {
    enter(e);
    if (!e || !tokens_out) return fail(e, -22, "sr_decode: null argument");
    const sr_config& c = e->c;
    if (B < 1 || B > c.max_batch || max_new < 1 || max_new > c.max_new_tokens || n_eos < 0 || n_eos > 32)
        return fail(e, -22, "sr_decode: B=%d max_new=%d n_eos=%d out of range", B, max_new, n_eos);
    (void)host_slots;   // slots were fixed by sr_prefill (kept in the signature for the continuous-batching scheduler)
    if (e->rows_mode) return fail(e, -22, "sr_decode: the engine is in continuous-batching mode (use sr_rows_step)");
    if (B != e->prefilled_B) return fail(e, -22, "sr_decode: B=%d but %d sequences were prefilled", B, e->prefilled_B);
    if (e->h_ctx_hi + max_new > c.max_ctx)
        return fail(e, -22, "sr_decode: context %d + %d new tokens exceeds max_ctx %d", e->h_ctx_hi, max_new, c.max_ctx);
    e->h_ctx_hi += max_new;
    hipStream_t s = (hipStream_t)stream;
    if (n_eos) SR_TRY((int)hipMemcpyAsync(e->d_eos, host_eos, n_eos * 4, hipMemcpyHostToDevice, s));
    const size_t V = c.t_vocab;
    if (logits_trace) SR_TRY((int)hipMemcpyAsync(logits_trace, e->d_logits, B * V * 4, hipMemcpyDeviceToDevice, s));
    // forced tokens are laid out [B][max_new] by the caller; the device log uses the engine's row stride
    const int* forced_dev = nullptr;
    if (forced) {
        if (max_new != c.max_new_tokens) return fail(e, -22, "teacher forcing requires max_new == max_new_tokens (%d)", c.max_new_tokens);
        forced_dev = forced;
    }
    Step st = make_step(B, n_eos, pad_id, nullptr);      // bookkeeping kernel + forward: k_step reduces the LM head's arg-max partials itself
    st.forced = forced_dev;
    if (int rc = begin_static_log(e, st, s)) return rc;
    hipGraphExec_t exec = nullptr;
    if (use_graph && !logits_trace && !forced) if (int rc = step_graph(e, STEP_GREEDY, st, &exec)) return rc;
    return decode_static(e, st, exec, max_new, logits_trace ? logits_trace + B * V : nullptr, tokens_out, s, steps_done);
}

// Sampled decode (temperature / top-k / top-p / repetition penalty of vllm_strategy.py:289-309), entirely on the device:
// the token of every step is drawn by k_sample from the logits the LM head left in HBM and fed back through k_step.
int sr_decode_sample(sr_engine* e, int B, int max_new, const int32_t* host_eos, int n_eos, int32_t pad_id, float temperature, int top_k,
                     float top_p, float rep_penalty, uint32_t seed, int32_t* tokens_out, int use_graph, void* stream, int* steps_done) {
    enter(e);
    if (!e || !tokens_out) return fail(e, -22, "sr_decode_sample: null argument");
    const sr_config& c = e->c;
    if (e->rows_mode) return fail(e, -22, "sr_decode_sample: the engine is in continuous-batching mode");
    if (B < 1 || B != e->prefilled_B || max_new < 1 || max_new > c.max_new_tokens || n_eos < 0 || n_eos > 32)
        return fail(e, -22, "sr_decode_sample: B=%d (prefilled %d) max_new=%d n_eos=%d out of range", B, e->prefilled_B, max_new, n_eos);
    if (!(temperature > 0.f) || top_k > 1024 || !(top_p > 0.f) || top_p > 1.f || !(rep_penalty > 0.f))
        return fail(e, -22, "sr_decode_sample: temperature > 0, top_k <= 1024 (<= 0: no top-k bound), 0 < top_p <= 1, repetition_penalty > 0 required");
    if (e->h_ctx_hi + max_new > c.max_ctx)
        return fail(e, -22, "sr_decode_sample: context %d + %d new tokens exceeds max_ctx %d", e->h_ctx_hi, max_new, c.max_ctx);
    e->h_ctx_hi += max_new;
    hipStream_t s = (hipStream_t)stream;
    if (n_eos) SR_TRY((int)hipMemcpyAsync(e->d_eos, host_eos, n_eos * 4, hipMemcpyHostToDevice, s));
    const bool rp = rep_penalty != 1.0f;
    Step st = make_step(B, n_eos, pad_id, e->d_sampled);      // one step: consume the drawn token, forward, draw the next
    st.mark = rp ? Step::MARK_CHOSEN : Step::MARK_NONE;
    st.tail = Step::TAIL_SAMPLE;
    st.sample = sample_args(e, B, false);
    st.sample.inv_temp = 1.0f / temperature; st.sample.top_k = top_k; st.sample.top_p = top_p; st.sample.rep_penalty = rep_penalty;
    st.sample.seen = rp ? e->d_seen : nullptr; st.sample.seed = seed;
    if (rp) SR_TRY(launch_mark_prompt(s, e->t_src, e->t_lastrow, e->d_seen, e->seen_words, B));
    if (e->lp_n >= 0) SR_TRY(launch_logprob_clear(s, B * c.max_new_tokens, e->lp_log, e->lp_ids, e->lp_tlp));
    if (int rc = enqueue_step_tail(e, st, s)) return rc;      // first token, from the prefill logits (and its record)
    hipGraphExec_t exec = nullptr;
    if (use_graph) if (int rc = step_graph(e, STEP_SAMPLED, st, &exec)) return rc;
    return decode_static(e, st, exec, max_new, nullptr, tokens_out, s, steps_done);
}

// Beam search (HF _beam_search, do_sample=False, early_stopping=False) over the G prompts of the last sr_prefill, W beams each, entirely on
// the device: the prompts are fanned out to W KV slots, and every step (one captured graph) feeds each row its chosen token (k_step),
// runs the forward, the row statistics, the group select (next beams, finished list, early stop, slot map, copy list) and the KV suffix
// copies.  The host polls the groups' stop flags every 16 steps and backtracks the parent / token trace once at the end.
static int ensure_beam_mem(sr_engine* e) {
    if (e->beam_mem) return 0;
    const sr_config& c = e->c;
    const size_t nb = beam_nb(c.t_vocab);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_part = take((size_t)MAXB * nb * (BEAM_MAXK + 1) * sizeof(BeamPart)), o_sc = take(MAXB * 4), o_tok = take(MAXB * 8),
                 o_tr = take((size_t)c.max_new_tokens * MAXB * sizeof(BeamTrace)), o_fin = take(MAXB * sizeof(BeamFin)), o_fn = take(MAXB * 4),
                 o_done = take(MAXB * 4), o_stop = take(MAXB * 4), o_eos = take(32 * 4), o_plen = take(MAXB * 4), o_fan = take(5 * MAXB * 4),
                 o_cp = take(MAXB * sizeof(int4));
    SR_TRY((int)hipMalloc(&e->beam_mem, off));
    char* m = static_cast<char*>(e->beam_mem);
    e->bm_part = reinterpret_cast<BeamPart*>(m + o_part); e->bm_scores = reinterpret_cast<float*>(m + o_sc);
    e->bm_tok = reinterpret_cast<long long*>(m + o_tok); e->bm_trace = reinterpret_cast<BeamTrace*>(m + o_tr);
    e->bm_fin = reinterpret_cast<BeamFin*>(m + o_fin); e->bm_fin_n = reinterpret_cast<int*>(m + o_fn); e->bm_done = reinterpret_cast<int*>(m + o_done);
    e->bm_stop = reinterpret_cast<int*>(m + o_stop); e->bm_eos = reinterpret_cast<int*>(m + o_eos); e->bm_plen = reinterpret_cast<int*>(m + o_plen);
    e->bm_fan = reinterpret_cast<int*>(m + o_fan); e->bm_copies = reinterpret_cast<int4*>(m + o_cp);
    return 0;
}

static int suffix_nx(int max_new) { return std::min(16, std::max(1, (max_new * 16 + 128 * (max_new / 8 + 2)) / 1024)); }

int sr_decode_beam(sr_engine* e, int G, int W, int R, int max_new, const int32_t* host_eos, int n_eos, int32_t pad_id, float length_penalty,
                   int32_t* tokens_out, float* scores_out, int32_t* lengths_out, float* logits_trace, int32_t* beam_trace, int use_graph,
                   void* stream, int* steps_done) {
    enter(e);
    if (!e || !tokens_out || !scores_out || !lengths_out) return fail(e, -22, "sr_decode_beam: null argument");
    const sr_config& c = e->c;
    if (e->rows_mode) return fail(e, -22, "sr_decode_beam: the engine is in continuous-batching mode");
    if (W < 1 || W > BEAM_MAXW) return fail(e, -22, "sr_decode_beam: num_beams W=%d outside 1..%d", W, BEAM_MAXW);
    if (R < 1 || R > W) return fail(e, -22, "sr_decode_beam: num_return_sequences R=%d outside 1..num_beams (%d)", R, W);
    if (n_eos < 0 || n_eos > 32 || (n_eos && !host_eos)) return fail(e, -22, "sr_decode_beam: n_eos=%d out of range", n_eos);
    const int K = std::max(2, 1 + n_eos) * W;
    if (K > BEAM_MAXK) return fail(e, -22, "sr_decode_beam: K = max(2, 1 + n_eos) * W = %d candidates exceed %d", K, BEAM_MAXK);
    if (G < 1 || G != e->prefilled_B) return fail(e, -22, "sr_decode_beam: G=%d but %d prompts were prefilled", G, e->prefilled_B);
    const int B = G * W;
    if (B > c.max_batch) return fail(e, -22, "sr_decode_beam: G*W = %d rows exceed max_batch %d", B, c.max_batch);
    if (max_new < 1 || max_new > c.max_new_tokens) return fail(e, -22, "sr_decode_beam: max_new=%d outside 1..%d", max_new, c.max_new_tokens);
    if (e->h_ctx_hi + max_new > c.max_ctx)
        return fail(e, -22, "sr_decode_beam: context %d + %d new tokens exceeds max_ctx %d", e->h_ctx_hi, max_new, c.max_ctx);
    if (c.t_vocab < K) return fail(e, -22, "sr_decode_beam: vocabulary %d smaller than K=%d", c.t_vocab, K);
    SR_TRY(ensure_beam_mem(e));
    hipStream_t s = (hipStream_t)stream;
    const size_t V = c.t_vocab;
    // ---- rows: group g's beam 0 keeps the prompt's KV slot, the others take free slots; every row starts at the prompt's state
    std::vector<int> used(e->n_slots, 0), rslot(B), st(5 * MAXB, 0), fan(5 * MAXB, 0), plen(MAXB, 0);
    for (int g = 0; g < G; ++g) used[e->pre_slot[g]] = 1;
    for (int g = 0, f = 0; g < G; ++g) {
        plen[g] = e->pre_len[g];
        for (int j = 0; j < W; ++j) {
            int sl = e->pre_slot[g];
            if (j) { while (used[f]) ++f; used[f] = 1; sl = f; fan[g * (W - 1) + j - 1] = sl; }
            const int r = g * W + j;
            rslot[r] = sl; st[r] = e->pre_len[g]; st[MAXB + r] = e->pre_pos[g]; st[2 * MAXB + r] = sl;
        }
        int* gr = fan.data() + MAXB + 4 * g;        // fan-out group: [src | L | first destination | destinations]
        gr[0] = e->pre_slot[g]; gr[1] = e->pre_len[g]; gr[2] = g * (W - 1); gr[3] = W - 1;
    }
    std::vector<float> sc0(B);
    for (int r = 0; r < B; ++r) sc0[r] = (r % W) ? -1.0e9f : 0.0f;
    std::vector<int> stop0(G, -1);
    SR_TRY((int)hipMemcpyAsync(e->d_ctx_len, st.data(), MAXB * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->d_pos, st.data() + MAXB, MAXB * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->d_slots, st.data() + 2 * MAXB, MAXB * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemsetAsync(e->d_finished, 0, MAXB * 4, s));
    SR_TRY((int)hipMemsetAsync(e->d_step, 0, MAXB * 4, s));
    SR_TRY((int)hipMemsetAsync(e->d_row_limit, 0x7f, MAXB * 4, s));
    SR_TRY((int)hipMemsetAsync(e->d_ngen, 0, MAXB * 4, s));
    SR_TRY((int)hipMemcpyAsync(e->bm_scores, sc0.data(), B * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemsetAsync(e->bm_fin_n, 0, MAXB * 4, s));
    SR_TRY((int)hipMemsetAsync(e->bm_done, 0, MAXB * 4, s));
    SR_TRY((int)hipMemcpyAsync(e->bm_stop, stop0.data(), G * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemsetAsync(e->bm_trace, 0xff, (size_t)max_new * B * sizeof(BeamTrace), s));
    if (n_eos) SR_TRY((int)hipMemcpyAsync(e->bm_eos, host_eos, n_eos * 4, hipMemcpyHostToDevice, s));
    SR_TRY((int)hipMemcpyAsync(e->bm_plen, plen.data(), MAXB * 4, hipMemcpyHostToDevice, s));
    // the prompt's logits row g -> rows g*W .. g*W+W-1 (descending g: a source row is read before any copy can overwrite it)
    for (int g = G - 1; g >= 0; --g)
        for (int j = 0; j < W; ++j)
            if (g * W + j != g)
                SR_TRY((int)hipMemcpyAsync(e->d_logits + (size_t)(g * W + j) * V, e->d_logits + (size_t)g * V, V * 4, hipMemcpyDeviceToDevice, s));
    if (W > 1) {
        int max_L = 0;
        for (int g = 0; g < G; ++g) max_L = std::max(max_L, e->pre_len[g]);
        SR_TRY((int)hipMemcpyAsync(e->bm_fan, fan.data(), 5 * MAXB * 4, hipMemcpyHostToDevice, s));
        KvFanoutArgs fa{e->kcache, e->vtcache, (long long)e->kv_layer_elems, c.t_layers, c.t_kv_heads, c.max_ctx, e->bm_fan, 0, 0, 0,
                        e->bm_fan + MAXB, G, max_L};
        SR_TRY(launch_kv_fanout(s, fa));
    }
    e->h_ctx_hi += max_new;
    e->prefilled_B = 0;            // the rows now hold beams: a new prefill is needed before the next decode
    BeamArgs ba{e->d_logits, (int)V, G, W, K, beam_nb((int)V), e->bm_part, e->bm_scores, e->bm_tok, e->bm_trace, B, e->bm_fin, e->bm_fin_n,
                e->bm_done, e->bm_stop, e->bm_eos, n_eos, pad_id, max_new, length_penalty, e->d_step, 0, e->d_slots, e->d_ctx_len, e->bm_plen,
                e->bm_copies};
    KvSuffixArgs ka{e->kcache, e->vtcache, (long long)e->kv_layer_elems, c.t_layers, c.t_kv_heads, c.max_ctx, e->bm_copies, B, suffix_nx(max_new)};
    Step step = make_step(B, 0, pad_id, e->bm_tok);      // one step: feed the chosen tokens, forward, select the next ones
    step.tail = Step::TAIL_BEAM; step.beam = &ba; step.suffix = &ka;
    hipGraphExec_t exec = nullptr;
    if (use_graph && !logits_trace) if (int rc = step_graph(e, STEP_BEAM, step, &exec)) return rc;
    if (logits_trace) SR_TRY((int)hipMemcpyAsync(logits_trace, e->d_logits, B * V * 4, hipMemcpyDeviceToDevice, s));
    if (int rc = enqueue_step_tail(e, step, s)) return rc;      // step 0, from the prompts' logits
    // steps 1 .. max_new - 1 (every one selects: none only records), with an early exit once every group has stopped
    int done = 1;
    if (int rc = run_steps(e, step, exec, 1, max_new, false, logits_trace ? logits_trace + B * V : nullptr, e->bm_done, G, s, &done)) return rc;
    // ---- the finished lists and the trace -> host; backtrack the R best hypotheses of every group
    std::vector<BeamFin> fin(B);
    std::vector<int> fin_n(G);
    std::vector<BeamTrace> tr((size_t)done * B);
    SR_TRY((int)hipMemcpyAsync(fin.data(), e->bm_fin, B * sizeof(BeamFin), hipMemcpyDeviceToHost, s));
    SR_TRY((int)hipMemcpyAsync(fin_n.data(), e->bm_fin_n, G * 4, hipMemcpyDeviceToHost, s));
    SR_TRY((int)hipMemcpyAsync(tr.data(), e->bm_trace, tr.size() * sizeof(BeamTrace), hipMemcpyDeviceToHost, s));
    if (beam_trace) SR_TRY((int)hipMemcpyAsync(beam_trace, e->bm_trace, (size_t)max_new * B * sizeof(BeamTrace), hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipStreamSynchronize(s));
    for (int g = 0; g < G; ++g) {
        if (fin_n[g] < R) return fail(e, -5, "sr_decode_beam: group %d finished %d hypotheses, %d requested", g, fin_n[g], R);
        for (int r = 0; r < R; ++r) {
            const BeamFin& f = fin[g * W + r];
            int32_t* out = tokens_out + ((size_t)g * R + r) * max_new;
            for (int k = 0; k < max_new; ++k) out[k] = pad_id;
            if (f.step < 0 || f.step >= done) return fail(e, -5, "sr_decode_beam: corrupt finished entry (step %d)", f.step);
            out[f.step] = f.token;
            for (int k = f.step - 1, b = f.parent; k >= 0; --k) {
                if (b < 0 || b >= W) return fail(e, -5, "sr_decode_beam: corrupt trace (step %d beam %d)", k, b);
                const BeamTrace& t = tr[(size_t)k * B + g * W + b];
                out[k] = t.token;
                b = t.parent;
            }
            scores_out[g * R + r] = f.score;
            lengths_out[g * R + r] = f.step + 1;
        }
    }
    if (steps_done) *steps_done = done;
    return 0;
}

int sr_rows_step(sr_engine* e, int n_steps, const int32_t* host_eos, int n_eos, int32_t pad_id, void* stream) {
    enter(e);
    if (!e || !e->rows_mode) return fail(e, -22, "sr_rows_step: call sr_rows_begin first");
    if (n_steps < 1 || n_eos < 0 || n_eos > 32) return fail(e, -22, "sr_rows_step: n_steps=%d n_eos=%d out of range", n_steps, n_eos);
    hipStream_t s = (hipStream_t)stream;
    if (n_eos) SR_TRY((int)hipMemcpyAsync(e->d_eos, host_eos, n_eos * 4, hipMemcpyHostToDevice, s));
    const int B = e->c.max_batch;
    const bool sampled = e->rows_perrow || e->rows_temp > 0.f;
    Step st = make_step(B, n_eos, pad_id, sampled ? e->d_sampled : nullptr);
    StepKind kind = STEP_GREEDY;
    if (sampled) { st.tail = Step::TAIL_SAMPLE; st.sample = sample_args(e, B, false); }
    if (e->rows_perrow) {          // per-row step: mark the consumed tokens, consume them, forward, draw every row under its own table entry
        kind = STEP_ROWS_PERROW;
        st.mark = Step::MARK_ROWS;
        st.sample.seen = e->rp_seen; st.sample.params = e->rp_rows; st.sample.seen_slot = e->d_slots;
    } else if (sampled) {          // sampled step: consume the drawn tokens, forward, draw the next ones for every row
        kind = STEP_ROWS_SAMPLED;
        st.sample.inv_temp = 1.0f / e->rows_temp; st.sample.top_k = e->rows_topk; st.sample.top_p = e->rows_topp; st.sample.seed = e->rows_seed;
    }
    hipGraphExec_t exec = nullptr;
    if (int rc = step_graph(e, kind, st, &exec)) return rc;
    for (int i = 0; i < n_steps; ++i) SR_TRY((int)hipGraphLaunch(exec, s));
    return 0;
}

int sr_rows_poll(sr_engine* e, int32_t* host_finished, int32_t* host_steps, void* stream) {
    enter(e);
    if (!e || !e->rows_mode || !host_finished || !host_steps) return fail(e, -22, "sr_rows_poll: bad argument / not in rows mode");
    hipStream_t s = (hipStream_t)stream;
    SR_TRY((int)hipMemcpyAsync(host_finished, e->d_finished, e->c.max_batch * 4, hipMemcpyDeviceToHost, s));
    SR_TRY((int)hipMemcpyAsync(host_steps, e->d_ngen, e->c.max_batch * 4, hipMemcpyDeviceToHost, s));
    SR_TRY((int)hipStreamSynchronize(s));
    return 0;
}

int sr_rows_read(sr_engine* e, int row, int32_t* dev_tokens_out, int n, void* stream) {
    enter(e);
    if (!e || !e->rows_mode || row < 0 || row >= e->c.max_batch || n < 0 || n > e->c.max_new_tokens)
        return fail(e, -22, "sr_rows_read: bad argument / not in rows mode");
    SR_TRY((int)hipMemcpyAsync(dev_tokens_out, e->d_tokens + (size_t)row * e->c.max_new_tokens, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// chunk partials of sr_op_token_logprobs (engines own theirs), grown to the largest call
static BeamPart* g_op_lp_part = nullptr;
static size_t g_op_lp_cap = 0;

int sr_logprobs(sr_engine* e, int top_n, void* stream) {
    enter(e);
    if (!e) return fail(e, -22, "sr_logprobs: null engine");
    if (top_n < -1 || top_n > LP_MAXN) return fail(e, -22, "sr_logprobs: top_n %d outside -1 (off) .. %d", top_n, LP_MAXN);
    hipStream_t s = (hipStream_t)stream;
    if (top_n >= 0 && !e->lp_mem) {
        const sr_config& c = e->c;
        const size_t n_rec = (size_t)c.max_batch * c.max_new_tokens, n_part = (size_t)MAXB * beam_nb(c.t_vocab) * LP_PW;
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
        const size_t o_lp = take(n_rec * 4), o_ids = take(n_rec * LP_MAXN * 4), o_tlp = take(n_rec * LP_MAXN * 4), o_slp = take(MAXB * 4),
                     o_sids = take(MAXB * LP_MAXN * 4), o_stlp = take(MAXB * LP_MAXN * 4), o_part = take(n_part * sizeof(BeamPart)),
                     o_parta = take(n_part * sizeof(BeamPart));
        void* mem = nullptr;
        SR_TRY((int)hipMalloc(&mem, off));
        char* m = static_cast<char*>(mem);
        e->lp_log = reinterpret_cast<float*>(m + o_lp); e->lp_ids = reinterpret_cast<int*>(m + o_ids); e->lp_tlp = reinterpret_cast<float*>(m + o_tlp);
        e->lps_lp = reinterpret_cast<float*>(m + o_slp); e->lps_ids = reinterpret_cast<int*>(m + o_sids); e->lps_tlp = reinterpret_cast<float*>(m + o_stlp);
        e->lp_part = reinterpret_cast<BeamPart*>(m + o_part); e->lp_part_adm = reinterpret_cast<BeamPart*>(m + o_parta);
        int rc = launch_logprob_clear(s, (int)n_rec, e->lp_log, e->lp_ids, e->lp_tlp);
        if (!rc) rc = (int)hipStreamSynchronize(s);
        if (rc) { (void)hipFree(mem); return fail(e, rc, "sr_logprobs: clearing the log failed with %d", rc); }
        e->lp_mem = mem;
    }
    e->lp_n = top_n;
    return 0;
}

int sr_rows_read_logprobs(sr_engine* e, int row, float* dev_lp, int32_t* dev_top_ids, float* dev_top_lp, int n, void* stream) {
    enter(e);
    if (!e || !dev_lp) return fail(e, -22, "sr_rows_read_logprobs: null argument");
    if (!e->lp_mem) return fail(e, -22, "sr_rows_read_logprobs: nothing was recorded (call sr_logprobs first)");
    if (row < 0 || row >= e->c.max_batch || n < 0 || n > e->c.max_new_tokens)
        return fail(e, -22, "sr_rows_read_logprobs: row %d / n %d outside 0..%d / 0..%d", row, n, e->c.max_batch - 1, e->c.max_new_tokens);
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const size_t at = (size_t)row * e->c.max_new_tokens;
    SR_TRY((int)hipMemcpyAsync(dev_lp, e->lp_log + at, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    if (dev_top_ids) SR_TRY((int)hipMemcpyAsync(dev_top_ids, e->lp_ids + at * LP_MAXN, (size_t)n * LP_MAXN * 4, hipMemcpyDeviceToDevice, s));
    if (dev_top_lp) SR_TRY((int)hipMemcpyAsync(dev_top_lp, e->lp_tlp + at * LP_MAXN, (size_t)n * LP_MAXN * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

int sr_op_token_logprobs(const float* logits, int64_t ld, int rows, int V, const int64_t* dev_tokens, const int32_t* row_map, int top_n, float* lp,
                         int32_t* tok_out, int32_t* top_ids, float* top_lp, void* stream) {
    if (!logits || !lp || rows < 1 || rows > MAXB || V < 16 || ld < V || (top_ids == nullptr) != (top_lp == nullptr))
        return fail(nullptr, -22, "sr_op_token_logprobs: rows %d outside 1..%d, V %d < 16, ld %lld < V or a null argument", rows, MAXB, V, (long long)ld);
    if (top_n < 0 || top_n > LP_MAXN) return fail(nullptr, -22, "sr_op_token_logprobs: top_n %d outside 0..%d", top_n, LP_MAXN);
    const size_t need = (size_t)rows * beam_nb(V) * LP_PW;
    if (need > g_op_lp_cap) {
        (void)hipDeviceSynchronize();
        if (g_op_lp_part) (void)hipFree(g_op_lp_part);
        g_op_lp_part = nullptr; g_op_lp_cap = 0;
        if (hipMalloc(&g_op_lp_part, need * sizeof(BeamPart)) != hipSuccess) return fail(nullptr, -12, "sr_op_token_logprobs: out of device memory");
        g_op_lp_cap = need;
    }
    LogprobArgs la{logits, (long long)ld, V, rows, top_n, row_map, g_op_lp_part, reinterpret_cast<const long long*>(dev_tokens), nullptr, nullptr, 0,
                   lp, tok_out, top_ids, top_lp};
    const int rc = launch_logprobs((hipStream_t)stream, la);
    if (rc) return fail(nullptr, rc, "sr_op_token_logprobs failed with %d", rc);
    return 0;
}

int sr_rows_set_cus(sr_engine* e, int n_cus, void* stream) {
    enter(e);
    if (!e || n_cus < 0) return fail(e, -22, "sr_rows_set_cus: bad argument");
    hipError_t r = hipMemsetD32Async((hipDeviceptr_t)(e->d_px + 10 * 16), n_cus, 1, (hipStream_t)stream);
    if (r != hipSuccess) return fail(e, (int)r, "sr_rows_set_cus: %s", hipGetErrorString(r));
    e->px_mode = n_cus > 0 ? 1 : 0;         // the decode step has two captured forms: the next steps replay the one for this stream
    return 0;
}

int sr_rows_abort(sr_engine* e, const int32_t* host_rows, int n, void* stream) {
    enter(e);
    if (!e || !e->rows_mode || !host_rows || n < 0) return fail(e, -22, "sr_rows_abort: bad argument / not in rows mode");
    unsigned mask[MAXB / 32] = {};
    for (int i = 0; i < n; ++i) {
        if (host_rows[i] < 0 || host_rows[i] >= e->c.max_batch || host_rows[i] >= MAXB) return fail(e, -22, "sr_rows_abort: row %d out of range", host_rows[i]);
        mask[host_rows[i] >> 5] |= 1u << (host_rows[i] & 31);
    }
    SR_TRY(launch_rows_abort((hipStream_t)stream, mask, e->d_finished));
    return 0;
}

int sr_decode_step(sr_engine* e, const int64_t* dev_last_ids, int B, float* dev_logits_out, int64_t* dev_next_ids, void* stream) {
    enter(e);
    if (!e) return fail(e, -22, "sr_decode_step: null engine");
    const sr_config& c = e->c;
    if (e->rows_mode) return fail(e, -22, "sr_decode_step: the engine is in continuous-batching mode");
    if (B < 1 || B != e->prefilled_B) return fail(e, -22, "sr_decode_step: B=%d but %d sequences were prefilled", B, e->prefilled_B);
    if (e->h_ctx_hi + 1 > c.max_ctx) return fail(e, -22, "sr_decode_step: context %d would exceed max_ctx %d", e->h_ctx_hi + 1, c.max_ctx);
    e->h_ctx_hi += 1;
    hipStream_t s = (hipStream_t)stream;
    // eos handling stays with the caller (n_eos = 0): a finished row is simply ignored by whoever samples.
    // One captured graph per (token source, B): step bookkeeping + forward + greedy ids, replayed from engine-owned buffers.
    Step st = make_step(B, 0, 0, dev_last_ids ? e->d_chosen : nullptr);
    st.tail = Step::TAIL_NEXT_IDS;
    hipGraphExec_t exec = nullptr;
    if (int rc = step_graph(e, dev_last_ids ? STEP_CALLER_CHOSEN : STEP_CALLER_GREEDY, st, &exec)) return rc;
    if (dev_last_ids) SR_TRY((int)hipMemcpyAsync(e->d_chosen, dev_last_ids, (size_t)B * 8, hipMemcpyDeviceToDevice, s));
    SR_TRY((int)hipGraphLaunch(exec, s));
    if (dev_logits_out) SR_TRY((int)hipMemcpyAsync(dev_logits_out, e->d_logits, (size_t)B * c.t_vocab * 4, hipMemcpyDeviceToDevice, s));
    if (dev_next_ids) SR_TRY((int)hipMemcpyAsync(dev_next_ids, e->d_next, (size_t)B * 8, hipMemcpyDeviceToDevice, s));
    return 0;
}

// ---------------------------------------------------------------------------------------------------- raster + ops
#define SR_WRAP(call) do { int rc_ = (call); if (rc_) return fail(nullptr, rc_, #call " failed with %d", rc_); return 0; } while (0)

int sr_mask_union(uint8_t* acc, const uint8_t* m, size_t n, void* stream) { SR_WRAP(launch_mask_union((hipStream_t)stream, acc, m, n)); }
int sr_resize_nearest_u8(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw, void* stream) {
    SR_WRAP(launch_resize_nearest_u8((hipStream_t)stream, src, sh, sw, dst, dh, dw));
}
int sr_resize_pil_u8(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw, int channels, int n_img, const int32_t* kk_h,
                     const int32_t* bounds_h, int ksize_h, const int32_t* kk_v, const int32_t* bounds_v, int ksize_v, uint8_t* tmp, void* stream) {
    SR_WRAP(launch_resize_pil_u8((hipStream_t)stream, src, sh, sw, dst, dh, dw, channels, n_img, kk_h, bounds_h, ksize_h, kk_v, bounds_v, ksize_v, tmp));
}
int sr_iou_counts(const uint8_t* p, const uint8_t* g, size_t n, int64_t* out2, void* stream) {
    SR_WRAP(launch_iou_counts((hipStream_t)stream, p, g, n, reinterpret_cast<long long*>(out2)));
}
int sr_iou_counts_batched(const uint8_t* p, const uint8_t* g, size_t n, int n_items, int64_t* out, void* stream) {
    SR_WRAP(launch_iou_counts_batched((hipStream_t)stream, p, g, n, n_items, reinterpret_cast<long long*>(out)));
}
int sr_render_overlay(uint8_t* img, int h, int w, const uint8_t* mask, int mh, int mw, const int32_t* boxes, int nb, void* stream) {
    SR_WRAP(launch_render_overlay((hipStream_t)stream, img, h, w, mask, mh, mw, boxes, nb));
}
int sr_op_gemm(const void* A, int lda, const void* W, int M, int N, int K, void* out, int ldo, const void* bias, const void* resid,
               const int32_t* rowmap, int epilogue, void* stream) {
    GemmArgs a{(const bf16_t*)A, lda, (const bf16_t*)W, M, N, K, out, ldo, (const bf16_t*)bias, (const bf16_t*)resid, rowmap,
               (epilogue & 0x100) ? 1 : 0, nullptr,      // bit 8 of `epilogue`: W is fragment-ordered (tiled16x64)
               (epilogue & 0x200) ? 256 : (epilogue & 0x400) ? 128 : 0};      // bits 9 / 10: force the 256- / 128-tile kernel
    a.gelu_fast = (epilogue & 0x1000) ? 2 : (epilogue & 0x800) ? 1 : 0;      // bit 11: EPI_GELU through gelu_fast_f; bit 12: ReLU instead of GELU
    SR_WRAP(launch_gemm((hipStream_t)stream, a, epilogue & 0xff));
}
// ---- SAM2 image path (socioreasoner_amd/sam2.py drives these; shapes and layouts: sam.hip, attention.hip)
int sr_op_attention(const void* q, int q_stride, const void* k, int k_stride, long long k_head_stride, const void* vt, int vt_stride,
                    long long vt_head_stride, void* out, int out_stride, const void* dev_work, int n_work, int n_heads, int group, float scale,
                    int causal, int head_dim, int q_tile, int v2_ok, void* stream) {
    AttnArgs a{(const bf16_t*)q, q_stride, (const bf16_t*)k, k_stride, k_head_stride, (const bf16_t*)vt, vt_stride, vt_head_stride,
               (bf16_t*)out, out_stride, (const AttnWork*)dev_work, n_work, n_heads, group, scale, causal, q_tile, v2_ok};
    SR_WRAP(launch_attn_prefill((hipStream_t)stream, a, head_dim));
}
int sr_op_sam_preprocess(const uint8_t* img, int h, int w, void* out_chw, int S, void* stream) {
    SR_WRAP(launch_sam_preprocess<bf16_t>((hipStream_t)stream, img, h, w, (bf16_t*)out_chw, S));
}
int sr_op_im2col(const void* chw, int S, int k, int stride, int pad, void* out, int ld, const int32_t* rowmap, void* stream) {
    SR_WRAP(launch_im2col<bf16_t>((hipStream_t)stream, (const bf16_t*)chw, S, k, stride, pad, (bf16_t*)out, ld, rowmap));
}
int sr_op_layernorm(const void* x, int ldx, const void* w, const void* b, void* out, int ldo, int rows, int C, float eps, void* stream) {
    SR_WRAP(launch_layernorm<bf16_t>((hipStream_t)stream, (const bf16_t*)x, ldx, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)out, ldo, rows, C, eps));
}
int sr_op_maxpool_win(const void* in, int ld_in, int C, int n_win, int ws, void* out, int ld_out, void* stream) {
    SR_WRAP(launch_maxpool_win<bf16_t>((hipStream_t)stream, (const bf16_t*)in, ld_in, C, n_win, ws, (bf16_t*)out, ld_out));
}
int sr_op_ew(const void* a, int lda, const void* b, int ldb, void* out, int ldo, int rows, int C, int mode, void* stream) {
    SR_WRAP(launch_ew<bf16_t>((hipStream_t)stream, (const bf16_t*)a, lda, (const bf16_t*)b, ldb, (bf16_t*)out, ldo, rows, C, mode));
}
int sr_op_transpose(const void* in, int ld_in, int rows, int cols, void* out, int ld_out, void* stream) {
    SR_WRAP(launch_transpose((hipStream_t)stream, (const bf16_t*)in, ld_in, rows, cols, (bf16_t*)out, ld_out));
}
int sr_op_upsample2x_add(const void* lat, const void* top, void* out, int H2, int C, int ld, void* stream) {
    SR_WRAP(launch_upsample2x_add<bf16_t>((hipStream_t)stream, (const bf16_t*)lat, (const bf16_t*)top, (bf16_t*)out, H2, C, ld));
}
int sr_op_pixel_shuffle_add(const void* g, int ldg, const void* feat, int ldf, void* out, int ldo, int W, int Co, void* stream) {
    SR_WRAP(launch_pixel_shuffle_add<bf16_t>((hipStream_t)stream, (const bf16_t*)g, ldg, (const bf16_t*)feat, ldf, (bf16_t*)out, ldo, W, Co));
}
int sr_op_mask_resize_or(const float* low, int ld, int col0, int n, int m, const float* score, uint8_t* acc, float* logits_out, int h, int w, void* stream) {
    SR_WRAP(launch_mask_resize_or((hipStream_t)stream, low, ld, col0, n, m, score, acc, logits_out, h, w));
}
int sr_op_gather_rows(const void* in, const int32_t* rows, void* out, int n, int H, void* stream) {
    SR_WRAP(launch_gather_rows((hipStream_t)stream, (const bf16_t*)in, rows, (bf16_t*)out, n, H));
}
// ---- SAM2 at the reference's precision (float32 storage and arithmetic: sam_f32.hip and sam.hip's float instantiations)
int sr_op_gemm_f32(const float* A, int lda, const float* W, int M, int N, int K, float* out, int ldo, const float* bias, const float* resid,
                   const int32_t* rowmap, int epilogue, void* stream) {
    const int e = epilogue & 0xff;
    if (e != EPI_STORE && e != EPI_RESID && e != EPI_GELU && e != EPI_F32) return -22;
    GemmF32Args a{A, lda, W, M, N, K, out, ldo, bias, e == EPI_RESID ? resid : nullptr, rowmap, e == EPI_GELU ? ((epilogue & 0x1000) ? 2 : 1) : 0};
    if (epilogue & 0x2000) return -22;      // (round 5's pre-split weight planes: measured slower, left the library in round 6)
    SR_WRAP(launch_gemm_f32((hipStream_t)stream, a));
}
int sr_op_attention_f32(const float* q, int q_stride, const float* k, int k_stride, const float* v, int v_stride, float* out, int out_stride,
                        const void* dev_work, int n_work, int n_heads, float scale, int head_dim, void* stream) {
    AttnF32Args a{q, q_stride, k, k_stride, v, v_stride, out, out_stride, (const AttnWork*)dev_work, n_work, n_heads, scale, 0};
    SR_WRAP(launch_attn_f32((hipStream_t)stream, a, head_dim));
}
int sr_op_attention_f32_causal(const float* q, int q_stride, const float* k, int k_stride, const float* v, int v_stride, float* out, int out_stride,
                               const void* dev_work, int n_work, int n_heads, float scale, int head_dim, void* stream) {
    AttnF32Args a{q, q_stride, k, k_stride, v, v_stride, out, out_stride, (const AttnWork*)dev_work, n_work, n_heads, scale, 1};
    SR_WRAP(launch_attn_f32((hipStream_t)stream, a, head_dim));
}
int sr_op_rmsnorm_f32(const float* x, int ldx, const float* w, float* out, int ldo, int rows, int C, float eps, void* stream) {
    SR_WRAP(launch_rmsnorm_f32((hipStream_t)stream, x, ldx, w, out, ldo, rows, C, eps));
}
int sr_op_rope_f32(float* x, int ld, const float* cos_t, const float* sin_t, int ldc, int rows, int n_heads, int head_dim, void* stream) {
    SR_WRAP(launch_rope_f32((hipStream_t)stream, x, ld, cos_t, sin_t, ldc, rows, n_heads, head_dim));
}
int sr_op_rope_table_f32(const float* inv_freq, int n_freq, const int32_t* pos, int n_pos, float* cos_t, float* sin_t, void* stream) {
    SR_WRAP(launch_rope_table_f32((hipStream_t)stream, inv_freq, n_freq, pos, n_pos, cos_t, sin_t));
}
int sr_op_sam_preprocess_f32(const uint8_t* img, int h, int w, float* out_chw, int S, void* stream) {
    SR_WRAP(launch_sam_preprocess<float>((hipStream_t)stream, img, h, w, out_chw, S));
}
int sr_op_im2col_f32(const float* chw, int S, int k, int stride, int pad, float* out, int ld, const int32_t* rowmap, void* stream) {
    SR_WRAP(launch_im2col<float>((hipStream_t)stream, chw, S, k, stride, pad, out, ld, rowmap));
}
int sr_op_layernorm_f32(const float* x, int ldx, const float* w, const float* b, float* out, int ldo, int rows, int C, float eps, void* stream) {
    SR_WRAP(launch_layernorm<float>((hipStream_t)stream, x, ldx, w, b, out, ldo, rows, C, eps));
}
int sr_op_maxpool_win_f32(const float* in, int ld_in, int C, int n_win, int ws, float* out, int ld_out, void* stream) {
    SR_WRAP(launch_maxpool_win<float>((hipStream_t)stream, in, ld_in, C, n_win, ws, out, ld_out));
}
int sr_op_ew_f32(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int rows, int C, int mode, void* stream) {
    SR_WRAP(launch_ew<float>((hipStream_t)stream, a, lda, b, ldb, out, ldo, rows, C, mode));
}
int sr_op_upsample2x_add_f32(const float* lat, const float* top, float* out, int H2, int C, int ld, void* stream) {
    SR_WRAP(launch_upsample2x_add<float>((hipStream_t)stream, lat, top, out, H2, C, ld));
}
int sr_op_pixel_shuffle_add_f32(const float* g, int ldg, const float* feat, int ldf, float* out, int ldo, int W, int Co, void* stream) {
    SR_WRAP(launch_pixel_shuffle_add<float>((hipStream_t)stream, g, ldg, feat, ldf, out, ldo, W, Co));
}
int sr_op_quant_mx(const void* x, int ldx, int M, int K, void* q, void* scales, int rows_pad, void* stream) {
    SR_WRAP(launch_quant_mx_act((hipStream_t)stream, (const bf16_t*)x, ldx, M, K, (unsigned char*)q, (unsigned char*)scales, rows_pad));
}
int sr_op_gemm_mx(const void* A8, int lda, const void* a_scale, int a_rows_pad, const void* W8, const float* w_scale, int M, int N, int K, void* out,
                  int ldo, const void* bias, const void* resid, int epilogue, void* stream) {
    GemmArgs a{(const bf16_t*)A8, lda, (const bf16_t*)W8, M, N, K, out, ldo, (const bf16_t*)bias, (const bf16_t*)resid, nullptr, 1, w_scale, 256,
               (const unsigned char*)a_scale, a_rows_pad};
    SR_WRAP(launch_gemm256_mx((hipStream_t)stream, a, epilogue & 0xff));
}
int sr_op_gemm_mx_vit(const void* A8, int lda, const void* a_scale, int a_rows_pad, const void* W8, const float* w_scale, int M, int N, int K, void* out,
                      int ldo, const void* bias, const void* resid, const int32_t* rowmap, const float* cos_t, const float* sin_t, void* vt, int vt_stride,
                      int head_dim, int epilogue, void* stream) {
    GemmArgs a{(const bf16_t*)A8, lda, (const bf16_t*)W8, M, N, K, out, ldo, (const bf16_t*)bias, (const bf16_t*)resid, rowmap, 1, w_scale, 256,
               (const unsigned char*)a_scale, a_rows_pad};
    a.vrope = VitRope{cos_t, sin_t, (bf16_t*)vt, vt_stride, N / 3, head_dim};
    SR_WRAP(launch_gemm256_mx((hipStream_t)stream, a, epilogue & 0xff));
}
int sr_op_rmsnorm_mx(const void* x, const void* w, void* q, void* scales, int rows, int C, int group, int rows_pad, float eps, void* stream) {
    SR_WRAP(launch_rmsnorm_mx((hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)w, (unsigned char*)q, (unsigned char*)scales, rows, C, eps, group, rows_pad));
}
int sr_op_quant_f8_rows(const void* w, int N, int K, void* w8, float* scale, void* stream) {
    SR_WRAP(launch_quant_f8_rows((hipStream_t)stream, (const bf16_t*)w, N, K, (unsigned char*)w8, scale));
}
int sr_op_gemv(const void* x, int ldx, const void* W, int M, int N, int K, void* out, int ksplit, int mode, void* stream) {
    GemvArgs a = gv((const bf16_t*)x, ldx, (const bf16_t*)W, M, N, K, out, (mode & 0xff) == GV_SWIGLU ? N / 2 : N);
    a.ksplit = ksplit;
    a.w_tiled = (mode & 0x100) ? 1 : 0;          // bit 8 of `mode`: W is fragment-ordered (tiled16x64)
    a.x_tiled = (mode & 0x800) ? 1 : 0;          // bit 11: x is fragment-ordered (tiled16x64 of [ceil16(M), K])
    if (M > 16) { if (int rc = op_px()) return rc; }
    a.px_counter = (g_op_px_mode || (sr_switches().gemv_xlds & 4)) ? g_op_px : nullptr;
    SR_WRAP(launch_gemv((hipStream_t)stream, a, mode & 0xff));
}
int sr_op_gemv_fused(const void* x, int ldx, const void* W, int M, int N, int K, void* out, int ldo, int mode, const void* bias,
                     const void* norm_w, float eps, const float* slabs, int n_slabs, void* x_out, float* amax_val,
                     int32_t* amax_idx, void* stream) {
    GemvArgs a = gv((const bf16_t*)x, ldx, (const bf16_t*)W, M, N, K, out, ldo);
    a.bias = (const bf16_t*)bias; a.norm_w = (const bf16_t*)norm_w; a.eps = eps; a.slabs = slabs; a.n_slabs = n_slabs;
    a.x_out = (bf16_t*)x_out; a.amax_val = amax_val; a.amax_idx = amax_idx;
    a.w_tiled = (mode & 0x100) ? 1 : 0;
    a.x_tiled = (mode & 0x800) ? 1 : 0;          // bit 11: x fragment-ordered; bit 12: SWIGLU output fragment-ordered
    a.out_tiled = (mode & 0x1000) ? 1 : 0;
    // the op-level callers (tests, probes; one stream at a time) share one process-wide counter block for the x-stationary kernels
    if (M > 16) { if (int rc = op_px()) return rc; }
    a.px_counter = (g_op_px_mode || (sr_switches().gemv_xlds & 4)) ? g_op_px : nullptr;
    SR_WRAP(launch_gemv((hipStream_t)stream, a, mode & 0xff));
}
int sr_op_gemv_set_cus(int n_cus, void* stream) {
    if (n_cus < 0) return fail(nullptr, -22, "sr_op_gemv_set_cus: negative CU count");
    if (int rc = op_px()) return rc;
    g_op_px_mode = n_cus > 0 ? 1 : 0;
    SR_WRAP((int)hipMemsetD32Async((hipDeviceptr_t)(g_op_px + 10 * 16), n_cus, 1, (hipStream_t)stream));
}
int sr_op_gemv_f32_blocks(int N, int M, int K, int has_norm) { return gemv_f32_blocks(N, M, K, has_norm); }
int sr_op_attn_decode(const void* qkv, int qkv_stride, const int32_t* pos, const int32_t* ctx_len, const void* rope_cos,
                      const void* rope_sin, void* kcache, void* vtcache, void* out, int out_stride, int B, int n_q_heads, int n_kv_heads, int ctx_max,
                      float scale, void* scores_scratch, void* stream) {
    int rc = attn_decode_prepare(ctx_max, n_q_heads / n_kv_heads);
    if (rc) return fail(nullptr, rc, "attn_decode_prepare failed with %d", rc);
    DecodeAttnArgs a{(const bf16_t*)qkv, qkv_stride, pos, ctx_len, nullptr, (const bf16_t*)rope_cos, (const bf16_t*)rope_sin, (bf16_t*)kcache, (bf16_t*)vtcache, (bf16_t*)out,
                     out_stride, B, n_q_heads, n_kv_heads, n_q_heads / n_kv_heads, ctx_max, scale, (bf16_t*)scores_scratch, 0, nullptr};
    SR_WRAP(launch_attn_decode((hipStream_t)stream, a));
}
int sr_op_rmsnorm(const void* x, const void* w, void* out, int rows, int H, float eps, void* stream) {
    SR_WRAP(launch_rmsnorm((hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)out, rows, H, eps));
}
int sr_op_resid_rmsnorm(void* x, const float* partials, int ksplit, const void* w, void* out, int rows, int H, float eps, void* stream) {
    SR_WRAP(launch_resid_rmsnorm((hipStream_t)stream, (bf16_t*)x, partials, ksplit, (const bf16_t*)w, (bf16_t*)out, rows, H, eps));
}
int sr_op_quant_f8(void* w_tiled, int N, int K, void* w8, float* scale, void* stream) {
    SR_WRAP(launch_quant_f8((hipStream_t)stream, (bf16_t*)w_tiled, N, K, (unsigned char*)w8, scale));
}
int sr_op_gemv_f8(const void* x, int ldx, const void* w8, const float* w_scale, int M, int N, int K, void* out, int ldo, int mode,
                  const void* bias, const void* norm_w, float eps, int ksplit, void* stream) {
    GemvArgs a{};
    a.x = (const bf16_t*)x; a.ldx = ldx; a.W = nullptr; a.W8 = (const unsigned char*)w8; a.w_scale = w_scale; a.w_tiled = 1;
    a.M = M; a.N = N; a.K = K; a.out = out; a.ldo = ldo; a.ksplit = ksplit > 0 ? ksplit : 1;
    a.bias = (const bf16_t*)bias; a.norm_w = (const bf16_t*)norm_w; a.eps = eps;
    a.x_tiled = (mode & 0x800) ? 1 : 0;          // bit 11: x fragment-ordered; bit 12: SWIGLU output fragment-ordered (as sr_op_gemv_fused)
    a.out_tiled = (mode & 0x1000) ? 1 : 0;
    if (M > 16) { if (int rc = op_px()) return rc; }
    a.px_counter = (g_op_px_mode || (sr_switches().gemv_xlds & 4)) ? g_op_px : nullptr;
    SR_WRAP(launch_gemv((hipStream_t)stream, a, mode & 0xff));
}
int sr_op_sample(const float* logits, int B, int V, float temperature, int top_k, float top_p, float rep_penalty, const uint32_t* seen,
                 uint32_t seed, const int32_t* step, int64_t* out, const float* blk_max, int n_blk, int blk_rows, void* stream) {
    if (!(temperature > 0.f)) return fail(nullptr, -22, "sr_op_sample: temperature must be > 0");
    SampleArgs a{logits, V, B, 1.0f / temperature, top_k, top_p, rep_penalty, seen, (V + 31) / 32, seed, step, reinterpret_cast<long long*>(out),
                 blk_max, n_blk, blk_rows};
    SR_WRAP(launch_sample((hipStream_t)stream, a));
}
int sr_op_kv_fanout(void* kcache, void* vtcache, int n_layers, int64_t layer_stride_elems, int n_kv_heads, int max_ctx, int src_slot,
                    const int32_t* dev_dst_slots, int d, int L, void* stream) {
    if (!kcache || !vtcache || !dev_dst_slots || src_slot < 0 || d < 1 || L < 1 || L > max_ctx || n_layers < 1 || n_kv_heads < 1 ||
        layer_stride_elems < (int64_t)(src_slot + 1) * n_kv_heads * max_ctx * 128)
        return fail(nullptr, -22, "sr_op_kv_fanout: bad arguments (src %d, d %d, L %d, max_ctx %d)", src_slot, d, L, max_ctx);
    KvFanoutArgs a{static_cast<bf16_t*>(kcache), static_cast<bf16_t*>(vtcache), (long long)layer_stride_elems, n_layers, n_kv_heads, max_ctx,
                   dev_dst_slots, src_slot, L, d, nullptr, 0, 0};
    SR_WRAP(launch_kv_fanout((hipStream_t)stream, a));
}
int sr_op_kv_suffix_copy(void* kcache, void* vtcache, int n_layers, int64_t layer_stride_elems, int n_kv_heads, int max_ctx,
                         const int32_t* dev_copies, int n, int max_len, void* stream) {
    if (!kcache || !vtcache || !dev_copies || n < 0 || n > 65535 || max_len < 0) return fail(nullptr, -22, "sr_op_kv_suffix_copy: bad argument");
    KvSuffixArgs a{static_cast<bf16_t*>(kcache), static_cast<bf16_t*>(vtcache), (long long)layer_stride_elems, n_layers, n_kv_heads, max_ctx,
                   reinterpret_cast<const int4*>(dev_copies), n, suffix_nx(max_len)};
    SR_WRAP(launch_kv_suffix((hipStream_t)stream, a));
}
int sr_op_beam_select(const float* logits, int G, int W, int V, const int32_t* host_eos, int n_eos, int step, int max_new, float length_penalty,
                      int32_t pad_id, float* dev_scores, void* dev_fin, int32_t* dev_fin_n, int32_t* dev_done, int32_t* dev_trace,
                      int64_t* dev_next_tok, void* stream) {
    const int K = std::max(2, 1 + n_eos) * W;
    if (!logits || !dev_scores || !dev_fin || !dev_fin_n || !dev_done || !dev_trace || !dev_next_tok || G < 1 || W < 1 || W > BEAM_MAXW ||
        G * W > MAXB || n_eos < 0 || n_eos > 32 || K > BEAM_MAXK || V < K || step < 0 || step >= max_new)
        return fail(nullptr, -22, "sr_op_beam_select: bad argument (G=%d W=%d V=%d n_eos=%d step=%d max_new=%d)", G, W, V, n_eos, step, max_new);
    hipStream_t s = (hipStream_t)stream;
    const int NB = beam_nb(V);
    void* scratch = nullptr;
    const size_t part_bytes = (size_t)G * W * NB * (K + 1) * sizeof(BeamPart);
    if (hipMalloc(&scratch, part_bytes + 64 * 4 + MAXB * 4) != hipSuccess) return fail(nullptr, -12, "sr_op_beam_select: out of memory");
    int* eos = reinterpret_cast<int*>(static_cast<char*>(scratch) + part_bytes);
    int rc = 0;
    if (n_eos) rc = (int)hipMemcpyAsync(eos, host_eos, n_eos * 4, hipMemcpyHostToDevice, s);
    BeamArgs a{logits, V, G, W, K, NB, static_cast<BeamPart*>(scratch), dev_scores, reinterpret_cast<long long*>(dev_next_tok),
               reinterpret_cast<BeamTrace*>(dev_trace), G * W, static_cast<BeamFin*>(dev_fin), dev_fin_n, dev_done, eos + 64,
               eos, n_eos, pad_id, max_new, length_penalty, nullptr, 0, nullptr, nullptr, nullptr, nullptr};
    a.step = step;                // (the stop step goes to scratch: the op reports the stop through dev_done)
    if (!rc) rc = launch_beam_rowstats(s, a);
    if (!rc) rc = launch_beam_select(s, a);
    if (!rc) rc = (int)hipStreamSynchronize(s);
    (void)hipFree(scratch);
    if (rc) return fail(nullptr, rc, "sr_op_beam_select failed with %d", rc);
    return 0;
}
int sr_op_argmax(const float* logits, int rows, int V, int32_t* out_idx, void* stream) {
    SR_WRAP(launch_argmax((hipStream_t)stream, logits, rows, V, out_idx));
}

}  // extern "C"
