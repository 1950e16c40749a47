"""Host reference of the bf16 prefill attention behind ``sr_op_attention`` (socioreasoner_amd/csrc/attention.hip: k_attn_prefill, k_attn_fewq,
k_attn_prefill2), plain torch on the CPU, driven by the kernels' own work items.  Not a test module: tests/test_host_attention_ref.py pins it
against torch's scaled_dot_product_attention and the oracle's attention lines, tests/test_gpu_attention_ops.py holds the kernels to it.

Inputs are what the C ABI takes: flat q / k / V^T buffers (element offsets from the pointer the kernel gets) with their strides, the work
items ``(q_row0, seq_len, q_off, k_row0, vt_off, q_len)`` (kernels.h AttnWork), ``n_heads``, ``group``, ``scale``, ``causal``, ``head_dim``
and ``q_tile``.  For an item and head h the queries are positions ``q_off .. min(q_off + q_tile, q_len or seq_len)`` of the sequence (buffer rows
``q_row0 + i``), the keys rows ``k_row0 .. k_row0 + seq_len`` of kv head ``h // group``, the values columns ``vt_off ..`` of V^T rows
``kvh * vt_head_stride + d * vt_stride``; the causal mask is ``key <= q_off + i``.

  * ``attention_exact``: float64 throughout, no intermediate rounding (``scale`` is the float32 value the ABI carries).
  * ``attention_eager``: HF eager's rounding points (attention.hip header, oracle/model_ref.py vit_attention / lm_attention):
    bf16(q k^T), bf16(. * scale) with a float32 scale, float32 softmax, bf16(P), bf16(P V).  Both matrix products are accumulated in
    float64 (``acc=torch.float64``, the default: no summation-order noise of the reference's own) or in float32 (``acc=torch.float32``:
    the very torch calls of the oracle, used by the host test that pins this file to it).

Both return ``(out, written)``: float64 ``[out_rows, out_stride]`` (zero where nothing is defined) and the boolean map of the elements
some work item writes.

The second half is the case table of tests/test_gpu_attention_ops.py and the generator of its inputs -- kept here so that the host test of
the reference's own noise floor walks exactly the cases, seeds and buffers the GPU test launches.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np
import torch

# kernels.h AttnWork / socioreasoner_amd/sam2.py _WORK
WORK = np.dtype([("q_row0", "<i4"), ("seq_len", "<i4"), ("q_off", "<i4"), ("k_row0", "<i4"), ("vt_off", "<i8"), ("q_len", "<i4"), ("pad", "<i4")])
KT = 64          # keys per staged tile of every kernel


def _bf(x: torch.Tensor) -> torch.Tensor:
    """one bf16 rounding point (float64 goes through float32 first, as an accumulator register does); float32 out"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def _gather(q, q_stride, k, k_stride, k_head_stride, vt, vt_stride, vt_head_stride, item, n_heads, group, head_dim, q_tile):
    q_row0, seq_len, q_off, k_row0, vt_off, q_len = (int(x) for x in item[:6])
    q_len = q_len if q_len > 0 else seq_len
    nq = min(q_off + q_tile, q_len) - q_off
    assert nq > 0 and seq_len > 0, item
    n_kv = n_heads // group
    Q = torch.as_strided(q, (nq, n_heads, head_dim), (q_stride, head_dim, 1), q_row0 * q_stride)
    K = torch.as_strided(k, (n_kv, seq_len, head_dim), (k_head_stride, k_stride, 1), k_row0 * k_stride)
    V = torch.as_strided(vt, (n_kv, head_dim, seq_len), (vt_head_stride, vt_stride, 1), vt_off)
    return Q, K, V, nq, q_off, q_row0, seq_len


def _run(mode, acc, q, q_stride, k, k_stride, k_head_stride, vt, vt_stride, vt_head_stride, work, n_heads, group, scale, causal, head_dim,
         q_tile, out_rows, out_stride):
    assert q.dim() == k.dim() == vt.dim() == 1 and n_heads % group == 0
    out = torch.zeros(out_rows, out_stride, dtype=torch.float64)
    written = torch.zeros(out_rows, out_stride, dtype=torch.bool)
    scale32 = torch.tensor(scale, dtype=torch.float32)
    kv_key, kv = None, None
    for item in sorted((tuple(int(x) for x in it[:6]) for it in work), key=lambda it: (it[3], it[4], it[1], it[2])):
        Q, K, V, nq, q_off, q_row0, seq_len = _gather(q, q_stride, k, k_stride, k_head_stride, vt, vt_stride, vt_head_stride, item, n_heads,
                                                       group, head_dim, q_tile)
        wide = torch.float64 if (mode == "exact" or acc == torch.float64) else torch.float32
        key = (int(item[3]), int(item[4]), seq_len)
        if key != kv_key:       # the items of one sequence follow each other in most launches: convert its K / V once
            kv_key = key
            kv = (K.to(wide).repeat_interleave(group, dim=0), V.to(wide).transpose(1, 2).repeat_interleave(group, dim=0))      # [H, L, D]
        kh, vh = kv
        qh = Q.to(wide).transpose(0, 1)                                                                                     # [H, nq, D]
        sc = qh @ kh.transpose(1, 2)
        mask = None
        if causal:
            mask = torch.arange(seq_len).unsqueeze(0) > (torch.arange(nq).unsqueeze(1) + q_off)
        if mode == "exact":
            sc = sc * float(scale32)
            if mask is not None:
                sc = sc.masked_fill(mask, float("-inf"))
            o = torch.softmax(sc, dim=-1) @ vh
        else:
            sc = _bf(sc)
            sc = _bf(sc * scale32)
            if mask is not None:
                sc = sc.masked_fill(mask, float("-inf"))
            pr = _bf(torch.softmax(sc, dim=-1))
            o = _bf(pr.to(wide) @ vh)
        rows = slice(q_row0, q_row0 + nq)
        out[rows, : n_heads * head_dim] = o.transpose(0, 1).reshape(nq, n_heads * head_dim).to(torch.float64)
        written[rows, : n_heads * head_dim] = True
    return out, written


def attention_exact(q, q_stride, k, k_stride, k_head_stride, vt, vt_stride, vt_head_stride, work, n_heads, group, scale, causal, head_dim,
                    q_tile, out_rows, out_stride):
    return _run("exact", torch.float64, q, q_stride, k, k_stride, k_head_stride, vt, vt_stride, vt_head_stride, work, n_heads, group, scale,
                causal, head_dim, q_tile, out_rows, out_stride)


def attention_eager(q, q_stride, k, k_stride, k_head_stride, vt, vt_stride, vt_head_stride, work, n_heads, group, scale, causal, head_dim,
                    q_tile, out_rows, out_stride, acc=torch.float64):
    assert acc in (torch.float64, torch.float32)
    return _run("eager", acc, q, q_stride, k, k_stride, k_head_stride, vt, vt_stride, vt_head_stride, work, n_heads, group, scale, causal,
                head_dim, q_tile, out_rows, out_stride)


# ================================================================================================ the GPU test's cases and their inputs
@dataclass(frozen=True)
class Case:
    name: str
    kernel: str                   # the kernel the launch must reach
    hd: int
    causal: bool
    q_tile: int
    v2_ok: int
    heads: int
    group: int
    seqs: tuple                   # (keys, queries): queries 0 = as many as keys, > 0 = pooled / few queries (the item's q_len)
    layout: str = "axis"          # "axis": sequences share one key axis (ViT / SAM2 V^T [kvh][d][all keys]); "slot": the engine's KV slots
    stress: str = ""              # "" or q4 / q0 / vmix / floor: judged against float64 only
    q_scale: float = 1.0
    seed: int = 0


LM_LENS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 449, 1100)
FULL_LENS = (1, 17, 64, 65, 200, 1024)
POOLED = ((256, 64), (1024, 256), (400, 100), (64, 16))
V2_LM_LENS = (32, 64, 65, 449, 463, 1100)


def _s(lens):
    return tuple((n, 0) for n in lens)


def _table():
    t = []
    for h, g in ((16, 8), (8, 4), (6, 3), (4, 1)):
        t.append(Case(f"lm_hd128_causal_{h}h_g{g}", "k_attn_prefill<128,causal>", 128, True, 64, 0, h, g, _s(LM_LENS), q_scale=1.5 if h == 16 else 1.0))
    for hd, h, g in ((80, 16, 1), (128, 8, 1), (128, 6, 2), (32, 8, 1), (32, 6, 2), (16, 8, 1), (16, 6, 2)):
        t.append(Case(f"full_hd{hd}_{h}h_g{g}", f"k_attn_prefill<{hd},full>", hd, False, 64, 0, h, g, _s(FULL_LENS), q_scale=2.0 if (hd, h) == (32, 8) else 1.0))
    t.append(Case("full_hd80_37_windows_of_64", "k_attn_prefill<80,full>", 80, False, 64, 0, 16, 1, _s((64,) * 37)))
    for hd in (80, 32):
        t.append(Case(f"pooled_hd{hd}_8h", f"k_attn_prefill<{hd},full>", hd, False, 64, 0, 8, 1, POOLED))
    for keys in (1, 63, 64, 65, 1000, 4096, 4100):
        t.append(Case(f"fewq_hd16_{keys}_keys", "k_attn_fewq<16,16>", 16, False, 16, 0, 8, 1, tuple((keys, nq) for nq in (1, 7, 9, 16))))
    for h, g in ((16, 8), (4, 4), (8, 4)):
        t.append(Case(f"v2_lm_hd128_causal_{h}h_g{g}", "k_attn_prefill2<128,causal>", 128, True, 64, 1, h, g, _s(V2_LM_LENS), layout="slot"))
    t.append(Case("v2_vit_hd80_2916_1024", "k_attn_prefill2<80,full>", 80, False, 128, 1, 16, 1, _s((2916, 1024))))
    t.append(Case("v2_vit_hd80_1024_4096", "k_attn_prefill2<80,full>", 80, False, 128, 1, 16, 1, _s((1024, 4096))))
    # stress rows (one-hot, uniform and mixed-magnitude inputs on both kernel generations): float64 criterion and finiteness only
    for st in ("q4", "q0", "vmix"):
        t.append(Case(f"stress_{st}_lm_hd128_449", "k_attn_prefill<128,causal>", 128, True, 64, 0, 4, 4, _s((449,)), stress=st))
        t.append(Case(f"stress_{st}_v2_lm_hd128_449", "k_attn_prefill2<128,causal>", 128, True, 64, 1, 4, 4, _s((449,)), layout="slot", stress=st))
        t.append(Case(f"stress_{st}_full_hd80_1024", "k_attn_prefill<80,full>", 80, False, 64, 0, 4, 1, _s((1024,)), stress=st))
        t.append(Case(f"stress_{st}_v2_vit_hd80_1024", "k_attn_prefill2<80,full>", 80, False, 128, 1, 4, 1, _s((1024,)), stress=st))
    t = tuple(replace(c, seed=1000 + i) for i, c in enumerate(t))
    assert set(OUTSIDE_THE_NOISE_FLOOR) <= {c.name for c in t}
    return tuple(replace(c, stress="floor") if c.name in OUTSIDE_THE_NOISE_FLOOR else c for c in t)


# Rows whose inputs put the REFERENCE's own summation-order noise (float32- against float64-accumulated products, measured on the CPU by
# tests/test_host_attention_ref.py) outside 2 bf16 ulp: the eager criterion cannot tell a kernel from a reference there, so they join the
# stress set (float64 criterion, exact facts, containment and tail masking still apply; the eager figures are recorded, not asserted).
OUTSIDE_THE_NOISE_FLOOR = {
    # 2.50 ulp at sequence 4 (63 keys), query position 7 (8 visible keys), head 2, d 14: -0.0864 (float32) / -0.0889 (float64) / -0.0869
    # exact.  All 80 differing elements of that (query, head) move together: with 8 keys one q.k^T sum that lands on a bf16 tie of the
    # score rounding (|s| ~ 16: one score ulp = 0.0625 * scale = 0.6 % of that key's P, largest P 0.22) rounds the other way under the
    # other accumulation width, and P.V carries the step into every channel.  Outputs of this short row are ~0.09 against a tensor rms of
    # 0.21 that floors the ulp at 2 ** -10, so the shift counts 2.5 of them.
    "lm_hd128_causal_8h_g4": "score-rounding tie at an 8-key causal row",
}


CASES = _table()

# q = 0 and identical V rows, power-of-two key counts, non-causal: the output is the V row, bit for bit
UNIFORM_CASES = (
    Case("uniform_prefill_hd32", "k_attn_prefill<32,full>", 32, False, 64, 0, 8, 1, ((64, 0), (1024, 100), (4096, 200)), seed=2000),
    Case("uniform_prefill_hd128", "k_attn_prefill<128,full>", 128, False, 64, 0, 6, 2, ((64, 0), (1024, 70), (4096, 64)), seed=2001),
    Case("uniform_fewq_hd16", "k_attn_fewq<16,16>", 16, False, 16, 0, 8, 1, ((64, 7), (1024, 16), (4096, 9)), seed=2002),
    Case("uniform_v2_vit_hd80", "k_attn_prefill2<80,full>", 80, False, 128, 1, 4, 1, ((64, 0), (1024, 0), (4096, 0)), seed=2003),
)


def _up(x, a):
    return (x + a - 1) // a * a


# bf16 bit patterns for the memory a kernel must not let through: quiet / signalling-range NaNs of both signs, +-max finite, +-inf
_GARBAGE = (0x7fc0, 0x7f7f, 0xffc1, 0xff7f, 0x7f81, 0x7f80, 0xffff, 0xff80)


def _bits(pattern, n):
    reps = (n + len(pattern) - 1) // len(pattern)
    return torch.from_numpy(np.tile(np.array(pattern, dtype=np.uint16), reps)[:n].view(np.int16).copy()).view(torch.bfloat16)


@dataclass
class Built:
    case: Case
    q: torch.Tensor
    k: torch.Tensor
    vt: torch.Tensor
    q_stride: int
    k_stride: int
    k_head_stride: int
    vt_stride: int
    vt_head_stride: int
    out_rows: int
    out_stride: int
    scale: float
    q_tile: int
    work: list                    # [(q_row0, seq_len, q_off, k_row0, vt_off, q_len)]
    seq_info: list                # per sequence: dict(q_row0, nq, keys, k_row0, vt_off)

    def ref_args(self, q_tile=None, work=None):
        c = self.case
        return (self.q, self.q_stride, self.k, self.k_stride, self.k_head_stride, self.vt, self.vt_stride, self.vt_head_stride,
                self.work if work is None else work, c.heads, c.group, self.scale, c.causal, c.hd, self.q_tile if q_tile is None else q_tile,
                self.out_rows, self.out_stride)

    def work_array(self, work=None):
        w = self.work if work is None else work
        arr = np.zeros(len(w), dtype=WORK)
        for i, it in enumerate(w):
            arr[i] = tuple(it) + (0,)
        return arr

    def written_map(self):
        """the output elements the work items define (what attention_exact / attention_eager return second)"""
        c = self.case
        written = torch.zeros(self.out_rows, self.out_stride, dtype=torch.bool)
        for q_row0, seq_len, q_off, _, _, q_len in self.work:
            written[q_row0: q_row0 + min(self.q_tile, (q_len or seq_len) - q_off), : c.heads * c.hd] = True
        return written


def cut(seq_info, q_tile, pooled_field):
    """work items of q_tile queries for the sequences of a Built"""
    work = []
    for si in seq_info:
        for q0 in range(0, si["nq"], q_tile):
            work.append((si["q_row0"] + q0, si["keys"], q0, si["k_row0"], si["vt_off"], si["nq"] if pooled_field(si) else 0))
    return work


def build(case: Case, tail="zero", uniform=False, q_tile=None) -> Built:
    """The launch of a case: seeded standard-normal bf16 q / k / V^T in buffers with row strides wider than the payload, sequences at
    unequal distances, work items in shuffled order.  ``tail``: what lies in the K rows and V^T columns between the end of a sequence and
    the next one (and the end of the allocation): "zero", or "garbage" -- NaN / inf / max-finite patterns where the kernel promises to
    mask them (v2_ok 0, and the K rows always), finite +-3e4 in the V^T tails of a v2_ok 1 launch.  Sequences lie where every precondition
    of the kernels holds (include/socior.h, sr_op_attention): 8-element q / k strides, V^T key runs starting on multiples of 4 (v2_ok: 8)
    elements and allocated to the next multiple of 4 (v2_ok: to the end of the last 64-key tile)."""
    c = case
    g = torch.Generator().manual_seed(c.seed)
    hd, H, n_kv = c.hd, c.heads, c.heads // c.group
    q_tile = q_tile or c.q_tile
    A = 8 if c.v2_ok else 4
    # ---- query rows: own packing, gaps of 0 / 3 / 1 rows nobody writes
    seq_info, row = [], 2
    for i, (keys, nq) in enumerate(c.seqs):
        seq_info.append({"q_row0": row, "nq": nq or keys, "keys": keys, "pooled": nq > 0})
        row += (nq or keys) + (0, 3, 1)[i % 3]
    out_rows = row + 2
    q_stride, out_stride = H * hd + 8, H * hd + 12
    q = torch.randn(out_rows * q_stride, generator=g)
    if c.stress == "q4":
        q = q * 4.0
    elif c.stress == "q0" or uniform:
        q = q * 0.0
    q = (q * c.q_scale).to(torch.bfloat16)
    # ---- keys / values
    if c.layout == "axis":
        pos, k_tail = A, []
        for i, si in enumerate(seq_info):
            start = _up(pos, A)
            k_tail.append((pos, start))
            si["k_row0"], si["vt_off"] = start, start
            pos = start + si["keys"] + (0, 5, 12)[i % 3]
            k_tail.append((start + si["keys"], pos))
        k_rows = pos
        total = _up(max(si["k_row0"] + _up(si["keys"], KT if c.v2_ok else 4) for si in seq_info), 8)
        total = max(total, _up(pos, 8))
        k_tail.append((pos, total))
        k_stride, k_head_stride = n_kv * hd + 16, hd
        vt_stride, vt_head_stride = total, hd * total
        k = torch.randn(k_rows * k_stride, generator=g).to(torch.bfloat16)
        vt = torch.randn(n_kv * hd * total, generator=g)
        if c.stress == "vmix":
            vt = vt * torch.pow(10.0, torch.rand(vt.shape, generator=g) * 6.0 - 3.0)
        vt = vt.to(torch.bfloat16)
        kv2, vt2 = k.view(k_rows, k_stride), vt.view(n_kv * hd, total)
        if uniform:
            for si in seq_info:
                a = si["vt_off"]
                vt2[:, a: a + si["keys"]] = vt2[:, a: a + 1].clone()
        for a, b in k_tail:
            if b > a:
                n = (min(b, k_rows) - a) * k_stride
                if n > 0:
                    kv2[a: min(b, k_rows)] = (_bits(_GARBAGE, n) if tail == "garbage" else torch.zeros(n, dtype=torch.bfloat16)).view(-1, k_stride)
                if tail == "garbage" and c.v2_ok:
                    fill = torch.tensor([3.0e4, -3.0e4], dtype=torch.bfloat16).repeat((b - a + 1) // 2)[: b - a].expand(n_kv * hd, b - a)
                elif tail == "garbage":
                    fill = _bits(_GARBAGE, n_kv * hd * (b - a)).view(n_kv * hd, b - a)
                else:
                    fill = torch.zeros(n_kv * hd, b - a, dtype=torch.bfloat16)
                vt2[:, a:b] = fill
    else:
        assert c.layout == "slot" and hd == 128
        ctx = _up(max(si["keys"] for si in seq_info), KT)
        n_slots = len(seq_info) + 1
        slots = torch.randperm(n_slots, generator=g).tolist()
        k_stride, k_head_stride = 128, ctx * 128
        vt_stride, vt_head_stride = ctx, 128 * ctx
        k = torch.randn(n_slots * n_kv * ctx * 128, generator=g).to(torch.bfloat16)
        vt = torch.randn(n_slots * n_kv * 128 * ctx, generator=g)
        if c.stress == "vmix":
            vt = vt * torch.pow(10.0, torch.rand(vt.shape, generator=g) * 6.0 - 3.0)
        vt = vt.to(torch.bfloat16)
        k4, vt4 = k.view(n_slots, n_kv, ctx, 128), vt.view(n_slots, n_kv, 128, ctx)
        for i, si in enumerate(seq_info):
            s, n = slots[i], si["keys"]
            si["k_row0"], si["vt_off"] = s * n_kv * ctx, s * n_kv * 128 * ctx
            if uniform:
                vt4[s, :, :, :n] = vt4[s, :, :, :1].clone()
            if ctx > n:
                if tail == "garbage":
                    k4[s, :, n:] = _bits(_GARBAGE, n_kv * (ctx - n) * 128).view(n_kv, ctx - n, 128)
                    if c.v2_ok:
                        vt4[s, :, :, n:] = torch.tensor([3.0e4, -3.0e4], dtype=torch.bfloat16).repeat((ctx - n + 1) // 2)[: ctx - n]
                    else:
                        vt4[s, :, :, n:] = _bits(_GARBAGE, n_kv * 128 * (ctx - n)).view(n_kv, 128, ctx - n)
                else:
                    k4[s, :, n:] = 0
                    vt4[s, :, :, n:] = 0
    work = cut(seq_info, q_tile, lambda si: si["pooled"])
    perm = torch.randperm(len(work), generator=g).tolist()
    work = [work[i] for i in perm]
    return Built(c, q, k, vt, q_stride, k_stride, k_head_stride, vt_stride, vt_head_stride, out_rows, out_stride,
                 float(np.float32(hd ** -0.5)), q_tile, work, seq_info)


def check_preconditions(b: Built, v2_ok: int):
    """Every launch the GPU test makes satisfies the documented contract of sr_op_attention (include/socior.h) and stays inside its
    buffers: asserted on the host before anything is launched."""
    c = b.case
    hd, H, n_kv = c.hd, c.heads, c.heads // c.group
    assert b.q_stride % 8 == 0 and b.k_stride % 8 == 0 and hd % 8 == 0 and b.k_head_stride % 8 == 0
    assert b.vt_stride % 4 == 0 and b.vt_head_stride % 4 == 0 and b.out_stride % 4 == 0 and b.out_stride >= H * hd and b.q_stride >= H * hd
    if v2_ok:
        assert b.vt_stride % 8 == 0 and b.vt_head_stride % 8 == 0 and H % 4 == 0
        assert (hd == 128 and c.group % 4 == 0 and c.causal and b.q_tile == 64) or (hd == 80 and c.group == 1 and not c.causal and b.q_tile == 128)
    for q_row0, seq_len, q_off, k_row0, vt_off, q_len in b.work:
        ql = q_len or seq_len
        assert seq_len >= 1 and 0 <= q_off < ql and q_off % b.q_tile == 0
        nq = min(b.q_tile, ql - q_off)
        assert q_row0 >= 0 and (q_row0 + nq) <= b.out_rows
        assert ((q_row0 + nq - 1) * b.q_stride + H * hd) <= b.q.numel()
        assert (k_row0 + seq_len - 1) * b.k_stride + (n_kv - 1) * b.k_head_stride + hd <= b.k.numel()
        run = _up(seq_len, KT if v2_ok else 4)
        assert vt_off % (8 if v2_ok else 4) == 0
        assert vt_off + (n_kv - 1) * b.vt_head_stride + (hd - 1) * b.vt_stride + run <= b.vt.numel()
        if v2_ok:
            tail = torch.as_strided(b.vt, (n_kv, hd, run), (b.vt_head_stride, b.vt_stride, 1), vt_off)
            assert bool(torch.isfinite(tail.float()).all())
