// KV prefix fan-out: a prompt admitted once serves n sampled sequences (reference: num_return_sequences, vLLM's n > 1 shares the prompt's KV
// blocks).  The engine prefills the prompt into the KV slot of its first fork; this kernel copies positions [0, L) of that slot into the
// slots of the other forks, every layer, both caches, in ONE launch:
//   kcache  [layer][slot][kvh][max_ctx][128]: the prefix of one (layer, kvh) is L x 256 B contiguous -> L x 16 chunks of 16 B;
//   vtcache [layer][slot][kvh][128][max_ctx]: 128 rows of L x 2 B (row stride max_ctx) -> ceil(L / 8) chunks per row, the last one a
//   partial chunk when L % 8 != 0 (its load reads the whole 16 B -- in bounds, max_ctx % 64 == 0 -- its stores write only the L % 8 elements).
// One thread per 16-byte chunk: the source is read once into registers and stored to every destination, so HBM traffic is (1 + d) x the prefix.
// Grid: x = chunks of one (layer, kvh) / 256, y = layer x kvh, z = fan-out group (one per prompt of an admission).  Positions >= L of a
// destination and the whole source slot are never written.
#include "kernels.h"

namespace {

constexpr int FT = 256;

__global__ __launch_bounds__(FT) void k_kv_fanout(KvFanoutArgs a) {
    int src = a.src, L = a.L, d = a.d;
    const int* dst = a.dst;
    if (a.groups) {                        // several prompts in one launch: [src | L | first destination index | d] per group
        const int* g = a.groups + 4 * blockIdx.z;
        src = g[0]; L = g[1]; dst += g[2]; d = g[3];
    }
    const int nK = L * 16, cpr = (L + 7) >> 3, nV = 128 * cpr;
    const int c = blockIdx.x * FT + threadIdx.x;
    if (c >= nK + nV || d <= 0) return;
    const int layer = blockIdx.y / a.n_kvh, h = blockIdx.y - layer * a.n_kvh;
    const size_t head = (size_t)a.max_ctx * 128;                 // elements of one (slot, kv head) in either cache
    const size_t slot_elems = head * a.n_kvh;
    const size_t base = (size_t)layer * (size_t)a.layer_stride + (size_t)h * head;
    bf16_t* cache;
    size_t off;
    int tail = 8;
    if (c < nK) {
        cache = a.kcache;
        off = (size_t)c * 8;
    } else {
        const int v = c - nK, r = v / cpr, q = v - r * cpr;
        cache = a.vtcache;
        off = (size_t)r * a.max_ctx + (size_t)q * 8;
        if (q == cpr - 1) tail = L - q * 8;
    }
    const uint4 x = *reinterpret_cast<const uint4*>(cache + base + (size_t)src * slot_elems + off);
    if (tail == 8) {
        for (int j = 0; j < d; ++j) *reinterpret_cast<uint4*>(cache + base + (size_t)dst[j] * slot_elems + off) = x;
    } else {
        const bf16_t* xs = reinterpret_cast<const bf16_t*>(&x);
        for (int j = 0; j < d; ++j) {
            bf16_t* p = cache + base + (size_t)dst[j] * slot_elems + off;
            for (int e = 0; e < tail; ++e) p[e] = xs[e];
        }
    }
}

}  // namespace

int launch_kv_fanout(hipStream_t s, const KvFanoutArgs& a) {
    const int n_groups = a.groups ? a.n_groups : 1, L = a.groups ? a.max_L : a.L;
    if (n_groups <= 0 || L <= 0) return 0;
    if (L > a.max_ctx || a.max_ctx % 64 || a.n_layers < 1 || a.n_kvh < 1 || n_groups > 65535) return -22;
    const int chunks = L * 16 + 128 * ((L + 7) >> 3);
    hipLaunchKernelGGL(k_kv_fanout, dim3((chunks + FT - 1) / FT, a.n_layers * a.n_kvh, n_groups), dim3(FT), 0, s, a);
    SR_CHECK_LAUNCH();
    return 0;
}
