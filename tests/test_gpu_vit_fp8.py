"""GPU tests of the opt-in fp8 vision tower (sr_config.v_weight_dtype = 2, Engine(vit_fp8="mx")): the fused RMSNorm + MX quantiser byte for byte,
the MX forms of the tower's GEMM epilogues against the float64-accumulated definition, the weight quantiser, and the tower end to end against
the definition (tests/vit_fp8_ref.py over oracle/model_ref.py) -- two small geometries, and the 3B tower at full depth against a fixture."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import vit_fp8_ref as VR
from tests.util import assert_bf16_close, bf16_compare, bits_to_f32, tile8

pytestmark = pytest.mark.gpu
EPI_STORE, EPI_RESID, EPI_GELU, EPI_VITQKV = 0, 1, 3, 6
SENT = -3855          # bf16 bit pattern 0xF0F1 as int16: what an output holds where nothing may write


@pytest.fixture(scope="module")
def L():
    from socioreasoner_amd import lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib.load()


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def record(name, payload):
    """the figures behind profiles/vit_fp8_parity.json: written only where SR_VIT_FP8_PARITY_JSON names a file"""
    path = os.environ.get("SR_VIT_FP8_PARITY_JSON")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    cur = json.load(open(path)) if os.path.exists(path) else {}
    cur[name] = payload
    json.dump(cur, open(path, "w"), indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------ k_rmsnorm_mx
@pytest.mark.parametrize("rows,Cw,group", [(1, 256, 1), (255, 256, 1), (257, 256, 1), (1, 1280, 1), (255, 1280, 1), (257, 1280, 1), (256, 256, 4), (256, 1280, 4)])
def test_rmsnorm_mx_equals_rmsnorm_then_quantiser_byte_for_byte(L, rows, Cw, group):
    """k_rmsnorm_mx against sr_op_rmsnorm followed by sr_op_quant_mx: element bytes and e8m0 scale bytes equal.  The reference RMSNorm is
    launched over at least 129 rows, which is where sr_op_rmsnorm takes the wave-per-row kernel the vision tower uses at EVERY row count
    (launch_rmsnorm per_wave; the block-per-row kernel of <= 128 decode rows sums the squares in another order); rows are independent, the
    first `rows` of them are compared.  group 4: the merger's view, 4 normalised rows = one GEMM row, scale block laid out for [rows / 4][4 C]."""
    g = torch.Generator().manual_seed(100 + rows + Cw)
    n_ref = max(rows, 129)
    x = torch.randn(n_ref, Cw, generator=g) * 3.0
    w = 1.0 + 0.25 * torch.randn(Cw, generator=g)
    x[0] = 5.0 * torch.sign(torch.randn(Cw, generator=g))          # constant magnitude: normalises to +-1 x w
    w[0:32] = 1.0                                                   # -> block 0 of row 0 has the exact power of two 1.0 as its maximum
    w[32:64] = torch.linspace(-1.99, 1.99, 32)                     # -> block 1 of row 0: maximum just under 2, element / X reaches 509: saturates at +-448
    if rows > 2:
        x[2] = 0.0                                                  # an all-zero row: every block all-zero (scale 2^-127)
    xb, wb = x.to(torch.bfloat16).cuda(), w.to(torch.bfloat16).cuda()
    xn = torch.empty(n_ref, Cw, dtype=torch.bfloat16, device="cuda")
    assert L.sr_op_rmsnorm(P(xb), P(wb), P(xn), n_ref, Cw, C.c_float(1e-6), sp()) == 0
    M, K = rows // group, group * Cw
    rows_pad = 256 if M <= 256 else 512
    q_ref = torch.zeros(M, K, dtype=torch.uint8, device="cuda")
    s_ref = torch.zeros(K // 128, rows_pad, 4, dtype=torch.uint8, device="cuda")
    assert L.sr_op_quant_mx(P(xn), K, M, K, P(q_ref), P(s_ref), rows_pad, sp()) == 0          # xn[:rows] viewed as [M][K]
    q = torch.full((M + 1, K), 0xA5, dtype=torch.uint8, device="cuda")
    s = torch.full((K // 128, rows_pad, 4), 0xA5, dtype=torch.uint8, device="cuda")
    assert L.sr_op_rmsnorm_mx(P(xb), P(wb), P(q), P(s), rows, Cw, group, rows_pad, C.c_float(1e-6), sp()) == 0
    torch.cuda.synchronize()
    assert torch.equal(q[:M].cpu(), q_ref.cpu())
    assert torch.equal(s[:, :M].cpu(), s_ref[:, :M].cpu())
    assert bool((q[M:] == 0xA5).all()) and bool((s[:, M:] == 0xA5).all())            # nothing past the last row
    # the inputs hold the cases they were built for (read off the reference's own output)
    r0 = xn[0].float().cpu()
    assert float(r0[0:32].abs().max()) == 1.0
    assert 1.98 < float(r0[32:64].abs().max()) < 2.0 and int((q_ref[0, 32:64].cpu() & 0x7F).max()) == 0x7E      # 0x7E = 448
    if rows > 2:
        m2, c2 = 2 // group, (2 % group) * Cw
        assert bool(((q_ref[m2, c2:c2 + Cw] & 0x7F) == 0).all()) and bool((s_ref[c2 // 128:(c2 + Cw) // 128, m2] == 0).all())      # +-0 elements, 2^-127


# ------------------------------------------------------------------------------------------------ weight quantiser
@pytest.mark.parametrize("N,K", [(768, 256), (1280, 3456)])
def test_row_major_weight_quantiser_equals_the_definition(L, N, K):
    """k_quant_f8_rows against oracle/model_ref.py QuantW: scales and the tiled8 image bit for bit; the bf16 master is left as it is.
    Row 5 is all zero (scale 1), the last 36 columns are zero (the padded intermediate size)."""
    from oracle import model_ref as MR
    w = rnd((N, K), 41, 0.03)
    w[5] = 0
    w[:, K - 36:] = 0
    wd = w.cuda()
    w8 = torch.zeros(N, K, dtype=torch.uint8, device="cuda")
    sc = torch.zeros(N, dtype=torch.float32, device="cuda")
    assert L.sr_op_quant_f8_rows(P(wd), N, K, P(w8), P(sc), sp()) == 0
    QW = MR.QuantW(w.float())
    assert torch.equal(sc.cpu(), QW.scale.float())
    assert torch.equal(w8.cpu(), tile8(QW.q8.view(torch.uint8)))
    assert torch.equal(wd.cpu(), w)


# ------------------------------------------------------------------------------------------------ MX epilogues
M_FULL = 268
CASES = [(768, 256, "vitqkv", 128), (3840, 1280, "vitqkv", 80), (1280, 3456, "store_rowmap", 0), (1280, 3456, "resid", 0), (5120, 5120, "gelu", 0)]


@functools.lru_cache(maxsize=None)
def _epilogue_case(N, K, kind, hd):
    """Inputs and the float64-accumulated definition for all 268 rows (rows are independent: the smaller launches compare their first M rows)."""
    from oracle import model_ref as MR
    x, w, b = rnd((M_FULL, K), 61), rnd((N, K), 62, 0.04), rnd((N,), 63, 0.1)
    QW = MR.QuantW(w.float())
    xq = MR.mx_quantize(x.float())[0]
    y = MR.r((xq.double() @ QW.q.double().t()).float() * QW.scale + b.float())       # the Linear's bf16 output
    d = {"x": x, "b": b, "w8": tile8(QW.q8.view(torch.uint8)), "wsc": QW.scale.float(), "y": y}
    if kind == "vitqkv":
        Cw, half = N // 3, hd // 2
        ang = torch.rand(M_FULL, half, generator=torch.Generator().manual_seed(64)) * 6.28
        d["cos"], d["sin"] = ang.cos(), ang.sin()
        # paired order (csrc/kernels.h vit_qk_perm): inside every 16-column tile, columns 0..7 are x1 of rotary pairs j..j+7, columns 8..15 their x2
        qk = y[:, :2 * Cw].reshape(M_FULL, 2 * Cw // hd, hd // 16, 2, 8)
        c, s = d["cos"].reshape(M_FULL, 1, hd // 16, 8), d["sin"].reshape(M_FULL, 1, hd // 16, 8)
        x1, x2 = qk[..., 0, :], qk[..., 1, :]
        o1, o2 = MR.r(x1 * c + (-x2) * s), MR.r(x2 * c + x1 * s)                       # float32 mul, mul, add, one rounding (hf:160-171)
        d["qk"] = torch.stack((o1, o2), dim=-2).reshape(M_FULL, 2 * Cw)
        d["vt"] = y[:, 2 * Cw:].t().contiguous()
    elif kind == "resid":
        d["res"] = rnd((M_FULL, N), 65)
        d["want"] = MR.r(d["res"].float() + y)
    elif kind == "gelu":
        d["want"] = MR.gelu_bf16(y)
    else:
        d["perm"] = torch.randperm(M_FULL + 5, generator=torch.Generator().manual_seed(66)).int()
        d["want"] = y
    return d


@pytest.mark.parametrize("M", [1, 140, 268])
@pytest.mark.parametrize("N,K,kind,hd", CASES)
def test_mx_epilogues_of_the_tower_against_the_definition(L, M, N, K, kind, hd):
    """The epilogues the LM path never instantiated in MX form, fed by the device quantiser: VITQKV (bias, 2-D rotary on the paired q / k channels,
    V written transposed), STORE through a destination row map, RESID at K = 3456 (27 k-tiles: an odd count), GELU at the merger's 5120 x 5120.
    Bounds (ulps / share of elements that differ) are those of test_gemm_mx_fp8_vs_oracle_definition for epilogues with the same number of
    roundings: 1 / 3 % for one rounding (V^T, STORE), 2 / 3 % with one more (q and k after the rotary, RESID), 3 / 5 % for a nonlinearity after
    the first rounding (GELU, as SWIGLU).  Outputs are sentinel-filled: they change only where the epilogue writes."""
    d = _epilogue_case(N, K, kind, hd)
    rows_pad = 512
    q = torch.zeros(M, K, dtype=torch.uint8, device="cuda")
    sc = torch.zeros(K // 128, rows_pad, 4, dtype=torch.uint8, device="cuda")         # (scale rows past M: valid e8m0 bytes, the tile's masked rows stay finite)
    assert L.sr_op_quant_mx(P(d["x"][:M].cuda()), K, M, K, P(q), P(sc), rows_pad, sp()) == 0
    w8, wsc, bias = d["w8"].cuda(), d["wsc"].cuda(), d["b"].cuda()
    rows_out = M + 5
    out = torch.full((rows_out, N), SENT, dtype=torch.int16, device="cuda")
    cos = sin = vt = rowmap = resid = None
    vts = (M + 7) // 8 * 8 + 8
    epi = {"vitqkv": EPI_VITQKV, "store_rowmap": EPI_STORE, "resid": EPI_RESID, "gelu": EPI_GELU}[kind]
    if kind == "vitqkv":
        cos, sin = d["cos"][:M].contiguous().cuda(), d["sin"][:M].contiguous().cuda()
        vt = torch.full((N // 3, vts), SENT, dtype=torch.int16, device="cuda")
    elif kind == "store_rowmap":
        rowmap = d["perm"][d["perm"] < rows_out][:M].contiguous().cuda()                # M distinct destination rows among M + 5
    elif kind == "resid":
        out[:M] = d["res"][:M].view(torch.int16).cuda()
        resid = out
    rc = L.sr_op_gemm_mx_vit(P(q), K, P(sc), rows_pad, P(w8), P(wsc), M, N, K, P(out), N, P(bias), P(resid), P(rowmap), P(cos), P(sin), P(vt), vts, hd, epi, sp())
    assert rc == 0
    torch.cuda.synchronize()
    o = out.cpu()
    val = lambda t: t.view(torch.bfloat16).float()
    if kind == "vitqkv":
        Cw = N // 3
        print(f"mx vitqkv {M}x{N}x{K}: q|k (ulp, share, abs)", bf16_compare(val(o[:M, :2 * Cw]), d["qk"][:M]), "V^T", bf16_compare(val(vt.cpu()[:, :M]), d["vt"][:, :M]))
        assert_bf16_close(val(o[:M, :2 * Cw]), d["qk"][:M], 2, 0.03, f"mx vitqkv q|k {M}x{N}x{K}")
        assert bool((o[:M, 2 * Cw:] == SENT).all()) and bool((o[M:] == SENT).all())     # V goes to V^T only; no row past M
        v = vt.cpu()
        assert_bf16_close(val(v[:, :M]), d["vt"][:, :M], 1, 0.03, f"mx vitqkv V^T {M}x{N}x{K}")
        m8 = (M + 7) // 8 * 8
        assert bool((v[:, m8:] == SENT).all())                                          # whole 8-row stores: up to the next multiple of 8 ...
        assert bool(torch.isfinite(val(v[:, M:m8])).all())                              # ... whose padding must be finite (attention multiplies it by 0)
    elif kind == "store_rowmap":
        rm = rowmap.cpu().long()
        print(f"mx store rowmap {M}x{N}x{K}: (ulp, share, abs)", bf16_compare(val(o[rm]), d["want"][:M]))
        assert_bf16_close(val(o[rm]), d["want"][:M], 1, 0.03, f"mx store rowmap {M}x{N}x{K}")
        rest = torch.ones(rows_out, dtype=torch.bool)
        rest[rm] = False
        assert bool((o[rest] == SENT).all())
    else:
        print(f"mx {kind} {M}x{N}x{K}: (ulp, share, abs)", bf16_compare(val(o[:M]), d["want"][:M]))
        assert_bf16_close(val(o[:M]), d["want"][:M], 2 if kind == "resid" else 3, 0.03 if kind == "resid" else 0.05, f"mx {kind} {M}x{N}x{K}")
        assert bool((o[M:] == SENT).all())


# ------------------------------------------------------------------------------------------------ the tower end to end, small geometries
def _engine(geom, **kw):
    from socioreasoner_amd.engine import Engine
    e = Engine(geom, max_patches=512, max_prefill_tokens=64, max_batch=1, max_ctx=64, max_new_tokens=8, **kw)
    e.load_synthetic_weights(seed=0)
    return e


@functools.lru_cache(maxsize=None)
def _small(name):
    """Everything the end-to-end tests of one geometry share: definition and bf16 oracle on the CPU (once), the engine's embeddings per mode."""
    from oracle import model_ref as MR
    from oracle import weights as WG
    cfg, geom = VR.small_configs(name)
    W = WG.LazyWeights(cfg, seed=0, fast=True)
    pix = VR.small_pixels(cfg)
    n0 = VR.GRIDS[0][1] * VR.GRIDS[0][2]
    d = {"cfg": cfg, "geom": geom, "definition": MR.vit_forward(VR.VitFp8Weights(W), cfg, pix, VR.GRIDS), "oracle": MR.vit_forward(W, cfg, pix, VR.GRIDS)}
    pd = pix.cuda()
    e = _engine(geom, vit_fp8="mx")
    d["fp8"] = e.vit_forward(pd, VR.GRIDS).clone()
    d["fp8_first_alone"] = e.vit_forward(pd[:n0].contiguous(), VR.GRIDS[:1]).clone()
    d["fp8_again"] = e.vit_forward(pd, VR.GRIDS).clone()
    e.close()
    e = _engine(geom)
    d["bf16"] = e.vit_forward(pd, VR.GRIDS).clone()
    e.close()
    e = _engine(geom, lm_fp8="mx")
    d["bf16_lm_mx"] = e.vit_forward(pd, VR.GRIDS).clone()
    e.close()
    e = _engine(geom, lm_fp8="mx", vit_fp8="mx")
    d["fp8_lm_mx"] = e.vit_forward(pd, VR.GRIDS).clone()
    e.close()
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("name", ["small128", "true80"])
def test_small_tower_fp8_against_the_definition(name):
    """Engine(vit_fp8="mx") against MR.vit_forward over the fp8 weight view, in the form of test_tiny_fp8_mx_prefill_against_oracle_definition: an
    e4m3 rounding that flips moves its element by 6 %, so two correct fp8 x fp8 forwards agree to about the perturbation the mode introduces
    (`quant_effect` = rms(definition - bf16 oracle), computed here); kernels and quantisers are pinned exactly at op level above."""
    d = _small(name)
    dfn, ora = d["definition"], d["oracle"]
    got, bf = d["fp8"].float().cpu(), d["bf16"].float().cpu()
    quant_effect, out_rms = VR.rms(dfn - ora), VR.rms(ora)
    st = {"rms": VR.rms(got - dfn), "mean": float((got - dfn).double().mean()), "quant_effect": quant_effect, "out_rms": out_rms,
          "engine_fp8_vs_engine_bf16": VR.rms(got - bf)}
    print(name, json.dumps(st))
    record(f"small_{name}", st)
    assert st["rms"] <= quant_effect, st
    assert abs(st["mean"]) <= 2e-3 * out_rms, st
    assert quant_effect >= 0.02 * out_rms, st                       # the mode is visible
    assert st["engine_fp8_vs_engine_bf16"] >= 0.5 * quant_effect, st   # the engine is not silently on the bf16 path


@pytest.mark.parametrize("name", ["small128", "true80"])
def test_small_tower_embedding_does_not_depend_on_the_rest_of_the_call(name):
    """The first image alone (128 rows) and next to the second (268 rows) gives the same embedding bit for bit: the MX path is taken at any row
    count; and a repeated call repeats its bits (the staging buffers carry nothing over)."""
    d = _small(name)
    n0 = VR.GRIDS[0][1] * VR.GRIDS[0][2] // 4
    assert torch.equal(d["fp8_first_alone"].view(torch.int16), d["fp8"][:n0].view(torch.int16))
    assert torch.equal(d["fp8_again"].view(torch.int16), d["fp8"].view(torch.int16))
    # the two switches are independent: the tower does not see the LM's weight format in either of its modes
    assert torch.equal(d["fp8_lm_mx"].view(torch.int16), d["fp8"].view(torch.int16))


@pytest.mark.parametrize("name", ["small128", "true80"])
def test_small_tower_switch_off_is_the_bf16_tower(name):
    """With the switch off: the bf16 oracle within the band the bf16 tower is held to wherever it is compared with MR.vit_forward (smoke(),
    tests/test_gpu_parity.py: 3 bf16 steps of the largest output), and the same bits whatever lm_weight_dtype is."""
    d = _small(name)
    got, ora = d["bf16"].float().cpu(), d["oracle"]
    assert float((got - ora).abs().max()) <= 3 * float(ora.abs().max()) * 2 ** -8
    assert torch.equal(d["bf16_lm_mx"].view(torch.int16), d["bf16"].view(torch.int16))


def test_reloading_one_matrix_requantises_it():
    """After sr_finalize_weights, one mlp.down_proj.weight is loaded again with other values and the weights finalised again: the bf16 masters
    are kept, so the matrix is quantised afresh and the output equals that of an engine given those weights from the start."""
    from oracle import weights as WG
    from socioreasoner_amd.engine import Engine
    cfg, geom = VR.small_configs("small128")
    name = "visual.blocks.1.mlp.down_proj.weight"
    other = WG.LazyWeights(cfg, seed=7, fast=True)[name] * 1.5
    pd = VR.small_pixels(cfg).cuda()
    e = _engine(geom, vit_fp8="mx")
    before = e.vit_forward(pd, VR.GRIDS).clone()
    e.load_weight(name, other)
    e.assert_ready()
    after = e.vit_forward(pd, VR.GRIDS).clone()
    e.close()
    W = WG.LazyWeights(cfg, seed=0, fast=True)
    f = Engine(geom, max_patches=512, max_prefill_tokens=64, max_batch=1, max_ctx=64, max_new_tokens=8, vit_fp8="mx")
    for n, _, _ in geom.param_specs():
        f.load_weight(n, other if n == name else W[n])
    f.assert_ready()
    fresh = f.vit_forward(pd, VR.GRIDS).clone()
    f.close()
    assert not torch.equal(before.view(torch.int16), after.view(torch.int16))
    assert torch.equal(after.view(torch.int16), fresh.view(torch.int16))


# ------------------------------------------------------------------------------------------------ full depth
def test_full_depth_3b_tower_fp8_against_the_definition_fixture(golden_dir):
    """The 3B tower, one 448 x 448 tile, synthetic weights seed 0, against tests/golden/vit_fp8_def3b.npz (tools/make_golden_vit_fp8.py: the
    definition and the bf16 oracle at full depth on the CPU, strided samples, and their quant_effect): rms(engine - definition) <= quant_effect.
    Recorded, not bounded: the distance to HF's float32 run (tests/golden/hf_truth3b.npz) as a multiple of HF-bf16's own, next to the bf16
    engine's.  Asserted only: fp8 is not CLOSER to float32 than 0.9 x the bf16 engine is."""
    from socioreasoner_amd import synthetic
    from socioreasoner_amd.config import geometry_3b
    from socioreasoner_amd.engine import Engine
    from tests.test_gpu_round3 import err
    from tests.test_gpu_round3 import record as record_truth
    f = np.load(os.path.join(golden_dir, "vit_fp8_def3b.npz"))
    g = np.load(os.path.join(golden_dir, "hf_truth3b.npz"))
    ps, hw, tile = int(f["pool_stride"][0]), int(f["hw"][0]), int(f["tile"][0])
    assert ps == int(g["pool_stride"][0]) and g["tile448_tiles"].tolist() == [tile] and int(g["tile448_hw"][0]) == hw
    grid = (1, hw // 14, hw // 14)
    geom = geometry_3b()
    out = {}
    for mode in ("bf16", "fp8_mx"):
        e = Engine(geom, max_patches=grid[1] * grid[2], max_prefill_tokens=64, max_batch=1, max_ctx=64, max_new_tokens=8, vit_fp8="mx" if mode == "fp8_mx" else False)
        e.load_synthetic_weights(seed=0)
        pix = e.patchify(torch.from_numpy(synthetic.tile_pixels(tile, hw, hw)).cuda())
        emb = e.vit_forward(pix, [grid])
        assert list(emb.shape) == f["shape"].tolist()
        out[mode] = emb.float().cpu().flatten()[::ps].clone()
        e.close()
    dfn, ora = bits_to_f32(f["definition"]), bits_to_f32(f["bf16_oracle"])
    quant_effect = float(f["quant_effect"][0])
    p16, p32 = bits_to_f32(g["tile448_pooler"]), torch.from_numpy(g["tile448_pooler_f32"])
    hf, e_bf, e_q = err(p16, p32), err(out["bf16"], p32), err(out["fp8_mx"], p32)
    res = {"engine_vs_definition": err(out["fp8_mx"], dfn), "quant_effect": quant_effect, "output_rms": float(f["output_rms"][0]),
           "engine_fp8_vs_engine_bf16": err(out["fp8_mx"], out["bf16"]), "engine_bf16_vs_bf16_oracle": err(out["bf16"], ora),
           "hf_bf16_vs_f32": hf, "hip_bf16_vs_f32": e_bf, "hip_fp8_mx_vs_f32": e_q,
           "rms_ratio_to_hf_bf16": {"bf16": e_bf["rms"] / hf["rms"], "fp8_mx": e_q["rms"] / hf["rms"]}}
    print("vit fp8 full depth", json.dumps(res))
    record("full3b_tile448", res)
    record_truth("vit_fp8_mx_tile448", res)
    assert res["engine_vs_definition"]["rms"] <= quant_effect, res
    assert e_q["rms"] >= 0.9 * e_bf["rms"], res
