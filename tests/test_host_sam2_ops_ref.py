"""CPU tests of the SAM2 pass references (tests/sam2_ops_ref.py) that tests/test_gpu_sam2_ops.py holds the HIP kernels to: each float64
reference equals a second, independently written form of its operation (1e-12, bit for bit for the index ops) and the oracle's own
pre- / post-processing; every launch of the GPU test satisfies the kernels' preconditions (include/socior.h) and the checker refuses one
broken copy per rule; and the float32 restatement's own distance to float64 -- the thing that sizes the bound a kernel gets on a case --
stays small enough that the bound still says something."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sam2_ref as SR
from tests import sam2_ops_ref as R

ID = lambda c: c.name


def cases(op, **kw):
    return [c for c in R.CASES if c.op == op and all(c.p.get(k) == v for k, v in kw.items())]


def live(b, name="out"):
    want, written = R.reference(b)[name]
    return want, written


# ------------------------------------------------------------------------------------------------ references against independent forms
@pytest.mark.parametrize("case", cases("layernorm"), ids=ID)
def test_layernorm_reference_is_the_two_pass_formula(case):
    b = R.build(case)
    p = b.p
    want, written = live(b)
    x = R.view(b, "x", p["rows"], p["ldx"])[:, : p["C"]].double()
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + p["eps"]) * b.bufs["w"][: p["C"]].double() + b.bufs["b"][: p["C"]].double()
    o = b.off.get("out", 0)
    got = want[o: o + p["rows"] * p["ldo"]].view(p["rows"], p["ldo"])
    assert float((got[:, : p["C"]] - y).abs().max()) <= 1e-12
    assert bool((got[:, p["C"]:] == 0).all()) and int(written.sum()) == p["rows"] * p["ldo"]
    if p.get("input") == "constant":          # a constant row normalises to 0: the output is the bias, whatever eps and the weight are
        assert torch.equal(got[:, : p["C"]], b.bufs["b"][: p["C"]].double().expand(p["rows"], p["C"]))


@pytest.mark.parametrize("case", cases("im2col"), ids=ID)
def test_im2col_reference_is_the_window_loop(case):
    b = R.build(case)
    p = b.p
    S, k, st, pad, ld, T = p["S"], p["k"], p["stride"], p["pad"], p["ld"], R.T_of(p)
    assert T == math.floor((S + 2 * pad - k) / st) + 1
    chw = b.bufs["chw"][: 3 * S * S].double().reshape(3, S, S)
    padded = F.pad(chw, (pad, pad, pad, pad))
    out = torch.zeros(T * T, ld, dtype=torch.float64)
    for ty in range(T):
        for tx in range(T):
            tok = ty * T + tx
            row = int(b.bufs["rowmap"][tok]) if "rowmap" in b.bufs else tok
            out[row, : 3 * k * k] = padded[:, ty * st: ty * st + k, tx * st: tx * st + k].reshape(-1)
    want, written = live(b)
    assert torch.equal(want[: T * T * ld].view(T * T, ld), out)
    assert int(written.sum()) == T * T * ld and not bool(written[T * T * ld:].any())


@pytest.mark.parametrize("case", cases("maxpool_win"), ids=ID)
def test_maxpool_reference_is_the_four_row_maximum(case):
    b = R.build(case)
    p = b.p
    C, n_win, ws, h2 = p["C"], p["n_win"], p["ws"], p["ws"] // 2
    x = R.view(b, "in", n_win * ws * ws, p["ld_in"])[:, :C].double().reshape(n_win, ws, ws, C)
    y = torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]]).amax(dim=0).reshape(n_win * h2 * h2, C)
    want, written = live(b)
    got = want[: n_win * h2 * h2 * p["ld_out"]].view(-1, p["ld_out"])
    assert torch.equal(got[:, :C], y)
    assert int(written.sum()) == n_win * h2 * h2 * C
    if p.get("negative"):
        assert float(y.max()) < 0


@pytest.mark.parametrize("case", cases("transpose") + cases("gather_rows"), ids=ID)
def test_index_op_references(case):
    b = R.build(case)
    p = b.p
    want, written = live(b)
    o = b.off.get("out", 0)
    if case.op == "transpose":
        src = b.bufs["in"].double().numpy()
        got = want.numpy()
        for r in (0, p["rows"] // 2, p["rows"] - 1):
            for c in (0, p["cols"] // 3, p["cols"] - 1):
                assert got[o + c * p["ld_out"] + r] == src[r * p["ld_in"] + c]
        assert int(written.sum()) == p["rows"] * p["cols"]
        assert torch.equal(want[written].view(p["cols"], p["rows"]), R.view(b, "in", p["rows"], p["ld_in"])[:, : p["cols"]].double().t())
    else:
        Hs = b.bufs["in"].numel() // (p["n_in"] + R.GUARD_ROWS)
        assert Hs * b.bufs["in"].element_size() == p["H"] * 2
        rows = b.bufs["rows"].tolist()
        for i, r in enumerate(rows):
            assert torch.equal(want[i * Hs: (i + 1) * Hs], b.bufs["in"][r * Hs: (r + 1) * Hs].double())
        assert int(written.sum()) == p["n"] * Hs
        if p["n"] > 2:
            assert len(set(rows)) < len(rows) and max(rows) == p["n_in"] - 1


@pytest.mark.parametrize("case", cases("upsample2x_add") + cases("pixel_shuffle_add"), ids=ID)
def test_scatter_references_are_the_definitions(case):
    b = R.build(case)
    p = b.p
    want, written = live(b)
    if case.op == "upsample2x_add":
        H2, C, ld = p["H2"], p["C"], p["ld"]
        lat, top = R.view(b, "lat", H2 * H2, ld).double(), R.view(b, "top", (H2 // 2) ** 2, ld).double()
        got = want[: H2 * H2 * ld].view(H2 * H2, ld)
        for y in range(H2):
            for x in range(H2):
                assert torch.equal(got[y * H2 + x, :C], lat[y * H2 + x, :C] + top[(y // 2) * (H2 // 2) + x // 2, :C])
        assert int(written.sum()) == H2 * H2 * C
    else:
        # ConvTranspose2d(kernel 2, stride 2) of a map whose per-pixel products are the GEMM's columns co * 4 + dy * 2 + dx
        W, Co = p["W"], p["Co"]
        g = R.view(b, "g", W * W, p["ldg"])[:, : 4 * Co].double()
        feat = R.view(b, "feat", 4 * W * W, p["ldf"])[:, :Co].double()
        x = torch.eye(W * W, dtype=torch.float64).reshape(1, W * W, W, W)                     # pixel i as channel i
        wt = g.reshape(W * W, Co, 2, 2)                                                         # [in = pixel][out = co][dy][dx]
        y = F.conv_transpose2d(x, wt, stride=2)[0].permute(1, 2, 0).reshape(4 * W * W, Co) + feat
        got = want[: 4 * W * W * p["ldo"]].view(-1, p["ldo"])[:, :Co]
        assert float((got - y).abs().max()) <= 1e-12
        assert int(written.sum()) == 4 * W * W * Co


@pytest.mark.parametrize("case", cases("ew"), ids=ID)
def test_ew_references(case):
    b = R.build(case)
    p = b.p
    rows, C, mode = p["rows"], p["C"], p["mode"]
    a = R.view(b, "a", rows, p["lda"])[:, :C].double()
    bb = R.view(b, "b", 1 if mode == 1 else rows, p["ldb"])[:, :C].double()
    y = {0: lambda: a + bb, 1: lambda: a + bb.expand(rows, C), 2: lambda: a.clamp_min(0.0),
         3: lambda: a * 0.5 * torch.special.erfc(-a / math.sqrt(2.0)), 4: lambda: a / (1.0 + torch.exp(-a)) * bb}[mode]()
    want, written = live(b)
    got = want[: rows * p["ldo"]].view(rows, p["ldo"])[:, :C]
    assert float((got - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))
    assert int(written.sum()) == rows * C
    if mode in (3, 4):
        assert float(a.min()) < -7.0 and float(a.max()) > 7.0


@pytest.mark.parametrize("case", cases("sam_preprocess"), ids=ID)
def test_preprocess_reference_is_the_oracles_in_float64(case):
    b = R.build(case)
    p = b.p
    h, w, S = p["h"], p["w"], p["S"]
    img = b.bufs["img"][: h * w * 3].reshape(h, w, 3)
    want, written = live(b)
    got = want[: 3 * S * S].view(3, S, S)
    oracle = SR.preprocess(img.numpy(), S)[0].double()                                        # float32 arithmetic
    assert float((got - oracle).abs().max()) <= 2e-5
    x = R.bilinear(img.permute(2, 0, 1).double().numpy() / 255.0, S, S, np.float64)
    y = (x - np.array(R.IMAGENET_MEAN)[:, None, None]) / np.array(R.IMAGENET_STD)[:, None, None]
    assert float((got - torch.from_numpy(y)).abs().max()) <= 1e-12
    assert int(written.sum()) == 3 * S * S
    if (h, w) == (S, S):
        assert float((got - ((img.permute(2, 0, 1).double() / 255.0 - torch.tensor(R.IMAGENET_MEAN, dtype=torch.float64).view(3, 1, 1))
                             / torch.tensor(R.IMAGENET_STD, dtype=torch.float64).view(3, 1, 1))).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", cases("mask_resize_or"), ids=ID)
def test_mask_reference_is_the_oracles_postprocess(case):
    b = R.build(case)
    p = b.p
    m, h, w, n, col0 = p["m"], p["h"], p["w"], p["n"], p["col0"]
    maps = b.bufs["low"].view(-1, p["ld"])[: m * m, col0: col0 + n].t().reshape(n, m, m)
    score = b.bufs["score"][col0: col0 + n]
    best_mask, masks, up = SR.postprocess(maps, score, (h, w))
    ref = R.reference(b)
    lg = ref["logits"][0][: n * h * w].view(n, h, w)
    assert float((lg - up.double()).abs().max()) <= 1e-4
    assert float((lg - torch.from_numpy(R.bilinear(maps.double().numpy(), h, w, np.float64))).abs().max()) <= 1e-12
    # first arg-max: no later column reaches the winner, no earlier one equals it
    best = R.best_of(b)
    assert all(float(score[k]) < float(score[best]) for k in range(best)) and all(float(score[k]) <= float(score[best]) for k in range(best, n))
    if p.get("tie"):
        assert sum(float(s) == float(score[best]) for s in score) >= 2 and (n < 3 or best > 0)
    init = b.outs["acc"].init
    acc = ref["acc"][0]
    assert bool((acc[h * w:] == R.GUARD_U8).all()) and not bool(ref["acc"][1][h * w:].any())
    assert bool((acc[: h * w][init[: h * w] != 0] == 1).all()) and 0 < int((init[: h * w] != 0).sum()) < h * w       # pre-set bits stay
    # the oracle's float32 mask of the best map agrees outside the band the GPU test exempts
    bound = R.bounds(b, "logits")["max_abs"]
    exempt = R.mask_exempt(b, bound)
    new = (acc[: h * w] != 0) & (init[: h * w] == 0)
    orc = masks[best].flatten().bool() & (init[: h * w] == 0)
    assert torch.equal(new[~exempt], orc[~exempt])
    if p.get("input") == "zero":
        assert torch.equal(acc, init.double()) and bound == 0.0


# ------------------------------------------------------------------------------------------------ rounding helper
def test_one_rounding_to_bf16():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(100000, generator=g, dtype=torch.float64) * torch.pow(2.0, torch.randint(-6, 6, (100000,), generator=g).double())
    got = R.round_bf16_bits(x).view(torch.bfloat16).double()
    lo = x.float().view(torch.int32).bitwise_and(-65536).view(torch.float32).double()          # truncation: the bf16 neighbour towards zero
    ulp = torch.pow(2.0, torch.floor(torch.log2(x.abs())) - 7)
    hi = lo + torch.sign(x) * ulp
    assert bool(((got == lo) | (got == hi)).all()) and bool(((got - x).abs() <= torch.minimum((lo - x).abs(), (hi - x).abs())).all())
    # a float64 just above a bf16 tie that float32 rounds ONTO the tie: one rounding goes up, two would go to even (down)
    tie = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8 - 2.0 ** -40], dtype=torch.float64)
    assert R.round_bf16_bits(tie).view(torch.bfloat16).double().tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -7]
    # the exact-op claim: float32 accumulation of two stored values rounds like the float64 sum
    for dt in (torch.bfloat16,):
        a = (torch.randn(100000, generator=g) * torch.pow(2.0, torch.randint(-6, 6, (100000,), generator=g).float())).to(dt)
        c = (torch.randn(100000, generator=g) * torch.pow(2.0, torch.randint(-6, 6, (100000,), generator=g).float())).to(dt)
        assert torch.equal((a.float() + c.float()).to(dt).view(torch.int16), R.round_bf16_bits(a.double() + c.double()))


# ------------------------------------------------------------------------------------------------ the table and the preconditions
def test_case_table_shape():
    names = [c.name for c in R.CASES]
    assert len(set(names)) == len(names)
    kernels = {(c.kernel, c.storage) for c in R.CASES}
    for want in ("k_layernorm_v<32,1>", "k_layernorm_v<64,1>", "k_layernorm_v<64,2>", "k_layernorm_v<64,3>", "k_layernorm<bf16_t>", "k_transpose",
                 "k_transpose_v", "k_gather_rows"):
        assert (want, "bf16") in kernels, want
    assert ("k_layernorm<float>", "f32") in kernels and ("k_mask_resize_or", "f32") in kernels and ("k_gather_rows", "f32") in kernels
    for k in ("k_sam_preprocess", "k_im2col", "k_maxpool_win", "k_ew", "k_upsample2x_add", "k_pixel_shuffle_add"):
        assert (k, "bf16") in kernels and (k, "f32") in kernels, k
    entries = {R.entry(c) for c in R.CASES}
    ops = ("sam_preprocess", "im2col", "layernorm", "maxpool_win", "ew", "transpose", "upsample2x_add", "pixel_shuffle_add", "mask_resize_or", "gather_rows")
    assert entries == {"sr_op_" + o for o in ops} | {"sr_op_" + o + "_f32" for o in R.F32_ENTRY}          # ten entry points and their seven float32 forms
    for mode in range(5):
        assert {c.p["rows"] * c.p["C"] for c in cases("ew", mode=mode)} >= {255, 256, 257}
    for a, s in R.TWINS:
        za, zs = R.build(R.BY_NAME[a]), R.build(R.BY_NAME[s])
        assert R.BY_NAME[a].kernel != R.BY_NAME[s].kernel
        wa, ma = R.reference(za)["out"]
        ws, ms = R.reference(zs)["out"]
        assert torch.equal(wa[ma], ws[ms])                       # the same logical input and output, through the other kernel


@pytest.mark.parametrize("case", R.CASES, ids=ID)
def test_every_launch_of_the_gpu_test_honours_the_preconditions(case):
    z, gb = R.build(case), R.build(case, garbage=True)
    R.check_preconditions(z)
    R.check_preconditions(gb)
    # the garbage variant differs only where the op must not look: same reference, same written map, same arguments
    rz, rg = R.reference(z), R.reference(gb)
    for name in rz:
        if z.outs[name].alias:                                    # in place: the untouched remainder of the buffer is the input's own
            assert torch.equal(rz[name][1], rg[name][1]) and torch.equal(rz[name][0][rz[name][1]], rg[name][0][rg[name][1]])
        else:
            assert torch.equal(rz[name][0], rg[name][0]) and torch.equal(rz[name][1], rg[name][1])
    assert [a for a in R.abi_args(z) if not isinstance(a, tuple)] == [a for a in R.abi_args(gb) if not isinstance(a, tuple)]
    if case.op not in ("sam_preprocess",) and not (case.op == "im2col"):
        assert any(not torch.equal(R.bits_of(z.bufs[k]), R.bits_of(gb.bufs[k])) for k in z.bufs), "nothing for the garbage to sit in"


def _broken(name, **changes):
    b = R.build(R.BY_NAME[name])
    for k, v in changes.items():
        if k == "off":
            b.off.update(v)
        elif k == "bufs":
            b.bufs.update({n: f(b.bufs[n]) for n, f in v.items()})
        elif k == "kernel":
            b.case = R.Case(b.case.name, b.case.op, b.case.storage, v, b.case.p, b.case.seed_name)
        else:
            b.p[k] = v
    return b


BROKEN = {
    "rows past the input": lambda: _broken("ln_bf16_C144_ldo192_r9", rows=12),
    "columns past the output row": lambda: _broken("ew_bf16_mode0_15x17", ldo=16),
    "output shorter than its rows": lambda: _broken("tr_vec_13x72", cols=80, ld_in=88),
    "vector kernel named, pointer misaligned": lambda: _broken("ln_bf16_C144_ldo192_r9", off={"x": 2}),
    "vector transpose named, cols % 8": lambda: _broken("tr_vec_13x72", cols=71),
    "scalar kernel named, launch vector-legal": lambda: _broken("ln_bf16_C144_ldo192_r9", kernel="k_layernorm<bf16_t>"),
    "odd H2": lambda: _broken("up_bf16_H6_C1", H2=5),
    "odd ws": lambda: _broken("mp_bf16_ws4_n1_C256", ws=3),
    "ld < 3 k k": lambda: _broken("im_bf16_S8_k7_ld64_rowmap", ld=146),
    "C > 1152": lambda: _broken("ln_f32_C1152", C=1153, ldx=1160),
    "ldo > 1152": lambda: _broken("ln_f32_C1152", ldo=1156),
    "H % 8": lambda: _broken("ga_bf16_n5_H64", H=60),
    "gather row out of range": lambda: _broken("ga_bf16_n5_H64", bufs={"rows": lambda r: torch.where(torch.arange(r.numel()) == 2, torch.full_like(r, 7), r)}),
    "negative gather row": lambda: _broken("ga_bf16_n5_H64", bufs={"rows": lambda r: r - 7}),
    "rowmap out of range": lambda: _broken("im_bf16_S8_k7_ld64_rowmap", bufs={"rowmap": lambda r: r + 1}),
    "rowmap with a repeated row": lambda: _broken("im_bf16_S8_k7_ld64_rowmap", bufs={"rowmap": lambda r: r.clamp_min(1)}),
    "mask columns past ld": lambda: _broken("mr_16_47x61_n3_c1_ld16", ld=3),
    "acc shorter than h * w": lambda: _broken("mr_16_47x61_n3_c1_ld16", h=60),
    "pixel shuffle ldg < 4 Co": lambda: _broken("ps_bf16_W3_Co8", ldg=31),
    "top map too small": lambda: _broken("up_bf16_H2_C300", H2=8),
    "image shorter than h * w * 3": lambda: _broken("pre_bf16_37x53_S64", h=40),
}


@pytest.mark.parametrize("rule", sorted(BROKEN), ids=lambda r: r.replace(" ", "_"))
def test_precondition_checker_refuses_a_broken_launch(rule):
    with pytest.raises(AssertionError):
        R.check_preconditions(BROKEN[rule]())


# ------------------------------------------------------------------------------------------------ the reference's own noise
ROUNDED = [c for c in R.CASES if not R.is_exact(c)]
# Caps on the float32 restatement's own distance to float64, per op, from the arithmetic and not from a kernel:
#   bf16 storage: a float32 result sits within ~2^-22 relative of float64 and changes the bf16 rounding only when float64 lies that close to
#     a rounding boundary of spacing 2^-8: a share of a few 2^-14 = 0.02 %.  Bilinear preprocessing multiplies the relative error of a
#     source coordinate (<= S * 2^-24) by the pixel-to-pixel contrast (up to 255 / 255 / std = 4.4, rms ~1): a few 2^-17 absolute, 0.25 % at
#     the outside.  A restatement may never be off by more than 1 ulp: then the bound of 1 ulp could not hold for a kernel either.
#   float32 storage: 64 float32 ulps of the tensor's rms (layernorm: ~sqrt(C) roundings in the statistics; erf / exp: a few ulps of a result
#     of a few rms), 1024 for the rows built to cancel (mean 100, deviation 0.1: the mean's rounding error, 100 * 2^-24, is divided by
#     0.1).  The resizes add the source coordinate's rounding -- three float32 operations on a value up to the source side, 4 * side * 2^-24
#     at the outside -- times the largest step between neighbouring source pixels, which is what a coordinate error is multiplied by.
SHARE_CAP, ULP_CAP = 0.0025, {"mean100": 1024.0}


def resize_cap(b):
    p = b.p
    if b.case.op == "sam_preprocess":
        src = b.bufs["img"][: p["h"] * p["w"] * 3].reshape(p["h"], p["w"], 3).double() / 255.0 / min(R.IMAGENET_STD)
        side = max(p["h"], p["w"])
    elif b.case.op == "mask_resize_or":
        src = b.bufs["low"].view(-1, p["ld"])[: p["m"] ** 2, p["col0"]: p["col0"] + p["n"]].reshape(p["m"], p["m"], p["n"]).double()
        side = p["m"]
    else:
        return 0.0
    step = max(float((src[1:] - src[:-1]).abs().max()) if src.shape[0] > 1 else 0.0, float((src[:, 1:] - src[:, :-1]).abs().max()) if src.shape[1] > 1 else 0.0)
    return 4.0 * side * 2.0 ** -24 * step


@pytest.mark.parametrize("case", ROUNDED, ids=ID)
def test_restatement_noise_leaves_the_gpu_bound_meaningful(case):
    b = R.build(case)
    name = "logits" if case.op == "mask_resize_or" else "out"
    bd = R.bounds(b, name)
    own = bd["own"]
    print(case.name, own, {k: v for k, v in bd.items() if k != "own"})
    if b.outs[name].kind == "bf16":
        assert own["max_ulp"] <= 1.0 + 1e-6 and own["share"] <= SHARE_CAP, own
        assert own["share"] <= bd["frac"] <= 4 * SHARE_CAP + 1e-3
    else:
        cap = ULP_CAP.get(case.p.get("input"), 64.0) * R.f32_ulp(bd["rms"]) + resize_cap(b)
        assert own["max_abs"] <= cap, (own, cap)
        assert own["max_abs"] <= bd["max_abs"] <= max(4 * cap, 2 * R.f32_ulp(bd["rms"]))
    if case.op == "mask_resize_or":
        exempt = R.mask_exempt(b, bd["max_abs"])
        share = float(exempt.double().mean())
        print(case.name, "exempt share", share)
        if case.p.get("input") == "zero":
            assert bd["max_abs"] == 0.0 and bool(exempt.all())     # every logit IS the threshold: judged exactly (no bit may be set)
        else:
            assert share <= 1e-3
            # no float32 / float64 disagreement outside the band
            v32 = R.restate32(b)["logits"][: case.p["n"] * case.p["h"] * case.p["w"]].view(case.p["n"], -1)[R.best_of(b)]
            v64 = R.mask_logits64(b)[R.best_of(b)].flatten()
            assert torch.equal((v32 > 0)[~exempt], (v64 > 0)[~exempt])


def test_exempted_share_of_the_gelu_tail():
    """below rms * 2^-8 float32's 1 + erf cancellation decides the last bit (judged by max_ulp alone); the floored mask still keeps at
    least 60 % of a draw over [-8, 8] (gelu(x) falls below it for x < -3.3, silu(x) for x < -6) for the differing-share criterion"""
    for case in cases("ew", mode=3) + cases("ew", mode=4):
        b = R.build(case)
        want, written = R.reference(b)["out"]
        keep = float(R.ew_floor_mask(want[written]).double().mean())
        assert keep >= 0.6, (case.name, keep)
