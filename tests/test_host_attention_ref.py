"""CPU tests of the prefill-attention reference (tests/attention_ref.py) that tests/test_gpu_attention_ops.py holds the HIP kernels to:
attention_exact is torch's float64 scaled_dot_product_attention; attention_eager with float32 accumulation is, bit for bit, the attention
lines of the oracle (oracle/model_ref.py vit_attention / lm_attention); and the reference's own summation-order noise -- float32- against
float64-accumulated products -- stays inside 2 bf16 ulp on 0.5 % of the elements for every case of the GPU matrix, a quarter of the
element share the GPU test allows the kernels.  The case table's launches are also checked against the documented contract of
sr_op_attention here, on the host, for every variant the GPU test launches."""
import pytest
import torch
import torch.nn.functional as F

from oracle import model_ref as MR
from tests import attention_ref as AR
from tests.util import bf16_compare


def test_work_item_layout_is_the_librarys():
    from socioreasoner_amd import sam2
    assert AR.WORK == sam2._WORK and AR.WORK.itemsize == 32


@pytest.mark.parametrize("causal,hd,H,G,seqs", [
    (False, 80, 4, 1, ((1, 0), (17, 0), (65, 0), (200, 0))),
    (False, 32, 6, 2, ((256, 64), (400, 100), (64, 16), (130, 0))),          # pooled queries
    (True, 128, 8, 4, ((1, 0), (63, 0), (64, 0), (129, 0), (300, 0))),
    (False, 16, 8, 1, ((1000, 7), (65, 16), (1, 9))),
])
def test_exact_equals_float64_sdpa(causal, hd, H, G, seqs):
    c = AR.Case("host", "-", hd, causal, 64 if hd != 16 else 16, 0, H, G, tuple(seqs), seed=7)
    b = AR.build(c)
    out, written = AR.attention_exact(*b.ref_args())
    assert int(written.sum()) == sum(si["nq"] for si in b.seq_info) * H * hd
    q2 = b.q.view(-1, b.q_stride).double()
    k2 = b.k.view(-1, b.k_stride).double()
    vt2 = b.vt.view(-1, b.vt_stride).double()
    n_kv = H // G
    for si in b.seq_info:
        nq, n = si["nq"], si["keys"]
        q = q2[si["q_row0"]: si["q_row0"] + nq, : H * hd].reshape(nq, H, hd).transpose(0, 1)
        k = k2[si["k_row0"]: si["k_row0"] + n, : n_kv * hd].reshape(n, n_kv, hd).transpose(0, 1).repeat_interleave(G, dim=0)
        v = vt2[:, si["vt_off"]: si["vt_off"] + n].reshape(n_kv, hd, n).transpose(1, 2).repeat_interleave(G, dim=0)
        mask = (torch.arange(n)[None] <= torch.arange(nq)[:, None]) if causal else None
        want = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=b.scale)          # [H, nq, hd]
        got = out[si["q_row0"]: si["q_row0"] + nq, : H * hd].reshape(nq, H, hd).transpose(0, 1)
        assert float((got - want).abs().max()) <= 1e-12, si
        assert bool(written[si["q_row0"]: si["q_row0"] + nq, : H * hd].all()) and not bool(written[:, H * hd:].any())


def test_eager_float32_is_the_oracles_vit_attention_lines():
    """oracle/model_ref.py vit_attention, the four lines inside its chunk loop, on the chunks of a packed buffer"""
    H, D = 16, 80
    lens = (64, 36, 200, 1)
    c = AR.Case("host", "-", D, False, 4096, 0, H, 1, tuple((n, 0) for n in lens), seed=11)      # one work item per chunk, as the oracle walks them
    b = AR.build(c)
    got, _ = AR.attention_eager(*b.ref_args(), acc=torch.float32)
    scaling = torch.tensor(D ** -0.5, dtype=torch.float32)
    for si in b.seq_info:
        n = si["keys"]
        q = b.q.view(-1, b.q_stride)[si["q_row0"]: si["q_row0"] + n, : H * D].float().reshape(n, H, D)
        k = b.k.view(-1, b.k_stride)[si["k_row0"]: si["k_row0"] + n, : H * D].float().reshape(n, H, D)
        v = b.vt.view(H, D, -1)[:, :, si["vt_off"]: si["vt_off"] + n].float().permute(2, 0, 1)
        qh, kh, vh = q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1)
        sc = MR.r(qh @ kh.transpose(1, 2))
        sc = MR.r(sc * scaling)
        pr = MR.r(torch.softmax(sc, dim=-1))
        want = MR.r(pr @ vh).transpose(0, 1).reshape(n, H * D)
        assert torch.equal(got[si["q_row0"]: si["q_row0"] + n, : H * D].float(), want), si


def test_eager_float32_is_the_oracles_lm_attention_lines():
    """oracle/model_ref.py lm_attention from repeat_kv to r(pr @ vh): causal, GQA, a prefill without past keys"""
    H, KVH, D = 16, 2, 128
    g = H // KVH
    for n in (1, 65, 300):
        c = AR.Case("host", "-", D, True, 4096, 0, H, g, ((n, 0),), seed=13 + n)
        b = AR.build(c)
        got, _ = AR.attention_eager(*b.ref_args(), acc=torch.float32)
        si = b.seq_info[0]
        q = b.q.view(-1, b.q_stride)[si["q_row0"]: si["q_row0"] + n, : H * D].float().reshape(n, H, D)
        k = b.k.view(-1, b.k_stride)[si["k_row0"]: si["k_row0"] + n, : KVH * D].float().reshape(n, KVH, D)
        v = b.vt.view(KVH, D, -1)[:, :, si["vt_off"]: si["vt_off"] + n].float().permute(2, 0, 1)
        s_new = s_tot = n
        kh = k.transpose(0, 1).repeat_interleave(g, dim=0)
        vh = v.transpose(0, 1).repeat_interleave(g, dim=0)
        qh = q.transpose(0, 1)
        scaling = torch.tensor(D ** -0.5, dtype=torch.float32)
        sc = MR.r(qh @ kh.transpose(1, 2))
        sc = MR.r(sc * scaling)
        past = s_tot - s_new
        iq = torch.arange(s_new).unsqueeze(1) + past
        ik = torch.arange(s_tot).unsqueeze(0)
        sc = sc.masked_fill(ik > iq, float("-inf"))
        pr = MR.r(torch.softmax(sc, dim=-1))
        want = MR.r(pr @ vh).transpose(0, 1).reshape(s_new, H * D)
        assert torch.equal(got[si["q_row0"]: si["q_row0"] + n, : H * D].float(), want), n


def test_work_item_cut_does_not_change_the_reference():
    """64-query items in shuffled order against one item per sequence: the same rows, bit for bit (float64 accumulation)"""
    c = AR.Case("host", "-", 128, True, 64, 0, 8, 4, ((449, 0), (65, 0), (1, 0)), seed=5)
    b = AR.build(c)
    a, wa = AR.attention_eager(*b.ref_args())
    whole = AR.cut(b.seq_info, 4096, lambda si: si["pooled"])
    w, ww = AR.attention_eager(*b.ref_args(q_tile=4096, work=whole))
    assert torch.equal(a, w) and torch.equal(wa, ww)


def test_case_table_shape():
    names = [c.name for c in AR.CASES]
    assert len(set(names)) == len(names)
    stress = [c for c in AR.CASES if c.stress]
    # the stress set: the twelve prescribed rows (three inputs x two shapes x two kernel generations) and at most a tenth of the table more
    assert len(stress) <= 12 + len(AR.CASES) // 10
    kernels = {c.kernel for c in AR.CASES}
    for want in ("k_attn_prefill<128,causal>", "k_attn_prefill<128,full>", "k_attn_prefill<80,full>", "k_attn_prefill<32,full>",
                 "k_attn_prefill<16,full>", "k_attn_fewq<16,16>", "k_attn_prefill2<128,causal>", "k_attn_prefill2<80,full>"):
        assert want in kernels, want


@pytest.mark.parametrize("case", AR.CASES + AR.UNIFORM_CASES, ids=lambda c: c.name)
def test_every_launch_of_the_gpu_test_honours_the_contract(case):
    """the buffers, strides, offsets and work items of every launch tests/test_gpu_attention_ops.py makes (zero and garbage tails, the
    v2_ok 0 twin of a v2_ok 1 row with its items re-cut to 64 queries) satisfy the preconditions written in include/socior.h and stay
    inside their allocations -- decided here, before any GPU sees them"""
    uniform = case in AR.UNIFORM_CASES
    for tail in ("zero", "garbage"):
        b = AR.build(case, tail=tail, uniform=uniform)
        AR.check_preconditions(b, case.v2_ok)
        if case.v2_ok:
            AR.check_preconditions(AR.build(case, tail=tail, uniform=uniform, q_tile=64), 0)
    z, gb = AR.build(case, uniform=uniform), AR.build(case, tail="garbage", uniform=uniform)
    assert z.work == gb.work and torch.equal(z.q.view(torch.int16), gb.q.view(torch.int16))
    # the two differ in the tails only: every element a work item may use is the same
    for si in z.seq_info:
        n_kv = case.heads // case.group
        ka = torch.as_strided(z.k, (n_kv, si["keys"], case.hd), (z.k_head_stride, z.k_stride, 1), si["k_row0"] * z.k_stride)
        kb = torch.as_strided(gb.k, (n_kv, si["keys"], case.hd), (z.k_head_stride, z.k_stride, 1), si["k_row0"] * z.k_stride)
        va = torch.as_strided(z.vt, (n_kv, case.hd, si["keys"]), (z.vt_head_stride, z.vt_stride, 1), si["vt_off"])
        vb = torch.as_strided(gb.vt, (n_kv, case.hd, si["keys"]), (z.vt_head_stride, z.vt_stride, 1), si["vt_off"])
        assert torch.equal(ka, kb) and torch.equal(va, vb)
    if not uniform:
        assert not torch.equal(z.vt.view(torch.int16), gb.vt.view(torch.int16)) or all(si["keys"] % 64 == 0 for si in z.seq_info)


@pytest.mark.parametrize("case", [c for c in AR.CASES if c.stress in ("", "floor")], ids=lambda c: c.name)
def test_reference_noise_floor_is_inside_the_gpu_bound(case):
    """float32- against float64-accumulated eager reference on the very inputs of the GPU case: at most 2 bf16 ulp on at most 0.5 % of the
    elements -- a quarter of the 2 % the GPU test grants the kernels, so that allowance is not consumed by the reference itself.  A row
    listed in attention_ref.OUTSIDE_THE_NOISE_FLOOR (judged against float64 only on the GPU) must really be outside: the list cannot
    be used to park a row the eager criterion could judge."""
    b = AR.build(case)
    lo, w1 = AR.attention_eager(*b.ref_args(), acc=torch.float32)
    hi, w2 = AR.attention_eager(*b.ref_args())
    assert torch.equal(w1, w2)
    mu, frac, mad = bf16_compare(lo[w1], hi[w1])
    print(f"{case.name}: float32- vs float64-accumulated reference: max {mu:.2f} ulp, {frac:.4%} of elements, max abs {mad:.3e}")
    if case.stress == "floor":
        assert mu > 2 + 1e-6 or frac > 0.005, (case.name, mu, frac, mad)
        return
    assert mu <= 2 + 1e-6 and frac <= 0.005, (case.name, mu, frac, mad)
