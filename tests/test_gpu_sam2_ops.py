"""Every SAM2 pass kernel (socioreasoner_amd/csrc/sam.hip: k_sam_preprocess, k_im2col, k_layernorm<bf16_t | float>, k_layernorm_v<32,1 |
64,1 | 64,2 | 64,3>, k_maxpool_win, k_ew, k_transpose, k_transpose_v, k_upsample2x_add, k_pixel_shuffle_add, k_mask_resize_or;
elementwise.hip: k_gather_rows) against float64, op by op, in both storage types.

Every call goes through ``lib.load().sr_op_*``; the inputs, the case table, the references and the bounds are tests/sam2_ops_ref.py (pinned
on the CPU by tests/test_host_sam2_ops_ref.py, which also checks every launch made here against the preconditions written in
include/socior.h before a GPU sees it).  Output buffers are pre-filled with a sentinel (0x7fc1 bf16, a NaN pattern float32, 0xAA bytes
behind ``acc``) and end in a guard region.  Per case:

  1. exact ops (im2col, maxpool_win, transpose, gather_rows, upsample2x_add, pixel_shuffle_add, ew modes 0 / 1 / 2, constant-row layernorm,
     and every pad column an op defines as zero) equal the float64 result rounded ONCE to the storage type, bit for bit;
  2. rounded ops in bf16 storage (preprocess, layernorm through its five kernels, ew 3 / 4): at most 1 bf16 ulp from the rounded float64
     result, on a share of at most 4 x the share the float32 restatement of the formula differs on (CPU, per case) + 1e-3; for ew 3 / 4 the
     share counts elements with |want| >= rms * 2^-8 only;
  3. float32 storage: |error| against float64 at most 4 x the float32 restatement's own on the case, at least 2 float32 ulps of the rms;
  4. the vector and the scalar kernels get the same logical input (the scalar one forced by a pointer 2 elements off): each meets its
     bound, the two transposes are bit-identical;
  5. mask_resize_or: ``logits_out`` by 3; ``acc`` equals the float64 mask outside the pixels whose float64 logit lies within that bound of
     0 (at most 0.1 % of a case); ties take the first maximum, a zero map sets no bit, pre-set bits stay, the bytes behind h * w keep
     their guard pattern, and ``logits_out`` NULL gives the same ``acc``;
  6. the output changes exactly where the reference writes and nowhere else (rows past the end, the columns [C, ld) of ops that do not
     own them, [rows, ld_out) of transpose, the prefix of an offset pointer, the guard region);
  7. NaN / inf in the input pad columns, in the rows past the end and around the scores change no output bit;
  8. refusals return -22 before any launch and leave the sentinel everywhere; rows = 0 / n = 0 return 0 and write nothing.

The measured figures of every case are printed and, when SR_SAM2_OPS_PARITY_JSON names a file, collected there (the run recorded in
profiles/sam2_ops_parity.json).
"""
import ctypes as C
import json
import os

import pytest
import torch

from tests import sam2_ops_ref as R

pytestmark = pytest.mark.gpu
ID = lambda c: c.name


@pytest.fixture(scope="module")
def L():
    from socioreasoner_amd import lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib.load()


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def record(name, payload):
    path = os.environ.get("SR_SAM2_OPS_PARITY_JSON")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    cur = json.load(open(path)) if os.path.exists(path) else {}
    cur[name] = payload
    json.dump(cur, open(path, "w"), indent=1, sort_keys=True)


def launch(L, b, logits=True, refuse=None):
    """one sr_op_* launch of a built case into its sentinel-filled (in place: input-filled) outputs; returns (rc, {output: bit patterns on the
    host}).  The launch is checked against the kernels' preconditions on the host first; ``refuse`` then replaces integer arguments by
    values the launcher must turn down before it launches anything."""
    R.check_preconditions(b)
    if refuse:
        b.p.update(refuse)
    dev = {name: o.init.clone().cuda() for name, o in b.outs.items()}
    for name, o in b.outs.items():
        if o.alias:
            dev[o.alias] = dev[name]
    for name, t in b.bufs.items():
        if name not in dev:
            dev[name] = t.cuda()

    def ptr(name):
        t = dev[name]
        assert t.data_ptr() % 256 == 0
        return C.c_void_p(t.data_ptr() + b.off.get(name, 0) * t.element_size())

    args = []
    for a in R.abi_args(b, logits):
        if isinstance(a, tuple):
            args.append(ptr(a[1]) if a[0] == "buf" else C.c_float(a[1]))
        else:
            args.append(a)
    rc = getattr(L, R.entry(b.case))(*args, sp())
    torch.cuda.synchronize()
    return rc, {name: dev[name].cpu() for name in b.outs}


def first(mask):
    return int(mask.nonzero()[0])


def containment(b, name, bits, written, fails, what=""):
    init = b.outs[name].init
    if not torch.equal(bits[~written], init[~written]):
        bad = (bits != init) & ~written
        fails.append(f"{what}{name}: {int(bad.sum())} elements outside what the op defines changed, first flat index {first(bad)} "
                     f"(pointer offset {b.off.get(name, 0)}, arguments {b.p})")
    if not b.outs[name].alias and b.outs[name].kind != "u8":
        left = (bits == init) & written
        if bool(left.any()):
            fails.append(f"{what}{name}: {int(left.sum())} elements the op defines still hold the sentinel, first flat index {first(left)}")


def judge(b, outs, fails, res):
    """criteria 1-3, 5 (logits) and 6 of the module docstring for the outputs of one launch"""
    c, ref = b.case, R.reference(b)
    for name in (n for n in outs if n != "acc"):
        want, written = ref[name]
        bits, kind = outs[name], b.outs[name].kind
        containment(b, name, bits, written, fails)
        got = R.values_of(bits, kind)
        if not bool(torch.isfinite(got[written]).all()):
            fails.append(f"{name}: non-finite output at flat index {first(~torch.isfinite(got) & written)}")
            continue
        pads = R.pad_mask(b)
        if pads is not None and bool((bits[pads] != 0).any()):
            fails.append(f"{name}: {int((bits[pads] != 0).sum())} pad elements are not +0, first flat index {first((bits != 0) & pads)}")
        if R.is_exact(c) or c.p.get("input") == "constant":
            wb = R.round_storage_bits(want, kind)
            bad = (bits != wb) & written
            res[name] = {"differing": int(bad.sum()), "elements": int(written.sum())}
            if bool(bad.any()):
                i = first(bad)
                fails.append(f"{name}: {int(bad.sum())} of {int(written.sum())} elements differ from the once-rounded float64 result, first flat "
                             f"index {i}: got {float(got[i])!r}, want {float(want[i])!r}")
            continue
        bd = R.bounds(b, name)
        m = R.measure(b, name, got, want, written)
        res[name] = {"kernel": m, "restatement": bd["own"], "bound": {k: v for k, v in bd.items() if k not in ("own", "rms")}, "rms": bd["rms"]}
        if kind == "bf16":
            if not (m["max_ulp"] <= bd["max_ulp"] + 1e-6 and m["share"] <= bd["frac"]):
                fails.append(f"{name}: max {m['max_ulp']:.2f} ulp, {m['share']:.4%} differ, max abs {m['max_abs']:.3e} "
                             f"(bound {bd['max_ulp']} ulp, {bd['frac']:.4%}; the float32 restatement's own: {bd['own']})")
        elif not m["max_abs"] <= bd["max_abs"]:
            i = first(((got - want).abs() == m["max_abs"]) & written)
            fails.append(f"{name}: max abs error {m['max_abs']:.3e} at flat index {i} (bound {bd['max_abs']:.3e}; the float32 restatement's own "
                         f"{bd['own']['max_abs']:.3e})")


def judge_acc(b, outs, fails, res):
    """criterion 5 for the running union"""
    p = b.p
    hw = p["h"] * p["w"]
    want, written = R.reference(b)["acc"]
    acc = outs["acc"]
    containment(b, "acc", acc, written, fails)
    if not bool((acc[:hw] <= 1).all()):
        fails.append(f"acc holds bytes other than 0 / 1, first pixel {first(acc[:hw] > 1)}")
    bound = R.bounds(b, "logits")["max_abs"]
    exempt = R.mask_exempt(b, bound) if p.get("input") != "zero" else torch.zeros(hw, dtype=torch.bool)
    bad = (acc[:hw].double() != want[:hw]) & ~exempt
    res["acc"] = {"differing": int(bad.sum()), "exempt": int(exempt.sum()), "pixels": hw, "set": int(want[:hw].sum()), "best": R.best_of(b)}
    if exempt.double().mean() > 1e-3:
        fails.append(f"acc: {int(exempt.sum())} of {hw} pixels lie within {bound:.2e} of the threshold (more than 0.1 %)")
    if bool(bad.any()):
        i = first(bad)
        fails.append(f"acc: {int(bad.sum())} of {hw} pixels differ from the float64 mask of map {R.best_of(b)} outside the exempt band, first pixel "
                     f"({i // p['w']}, {i % p['w']}): got {int(acc[i])}, want {int(want[i])}, float64 logit {float(R.mask_logits64(b)[R.best_of(b)].flatten()[i])!r}")


@pytest.mark.parametrize("case", R.CASES, ids=ID)
def test_sam2_pass_kernel_against_float64(L, case):
    """(module docstring) criteria 1-3 and 5-7 for one row of the case table; every failed criterion is reported"""
    b = R.build(case)
    rc, outs = launch(L, b)
    assert rc == 0, rc
    fails, res = [], {"kernel": case.kernel, "entry": R.entry(case), "arguments": {k: v for k, v in b.p.items()}}
    judge(b, outs, fails, res)
    if case.op == "mask_resize_or":
        judge_acc(b, outs, fails, res)
        rc, quiet = launch(L, R.build(case), logits=False)
        if rc != 0 or not torch.equal(quiet["acc"], outs["acc"]):
            fails.append(f"logits_out NULL gives another acc (rc {rc}): {int((quiet['acc'] != outs['acc']).sum())} bytes")
        if not torch.equal(quiet["logits"], b.outs["logits"].init):
            fails.append("logits_out NULL: the buffer that was not passed changed")
    # ---- 7. what lies in the pad columns and past the end must not leak
    gb = R.build(case, garbage=True)
    rc, outs_g = launch(L, gb)
    ref = R.reference(b)
    for name in outs:
        written = ref[name][1]
        containment(gb, name, outs_g[name], written, fails, "garbage run: ")
        if rc != 0 or not torch.equal(outs_g[name][written], outs[name][written]):
            fails.append(f"NaN / inf outside the live elements leak into {name} (rc {rc}): {int((outs_g[name] != outs[name])[written].sum())} elements change")
    res["failed"] = fails
    print(case.name, json.dumps(res))
    record(case.name, res)
    assert not fails, case.name + ":\n  " + "\n  ".join(fails)


@pytest.mark.parametrize("vec,scalar", R.TWINS, ids=lambda n: n)
def test_vector_and_scalar_kernels_agree(L, vec, scalar):
    """criterion 4: the same logical input through k_layernorm_v / k_transpose_v and through k_layernorm<bf16_t> / k_transpose"""
    bv, bs = R.build(R.BY_NAME[vec]), R.build(R.BY_NAME[scalar])
    assert bv.case.kernel != bs.case.kernel
    (rv, ov), (rs, os_) = launch(L, bv), launch(L, bs)
    assert rv == 0 and rs == 0, (rv, rs)
    fails = []
    for b, o in ((bv, ov), (bs, os_)):
        res = {}
        judge(b, o, fails, res)
    wv, ws = R.reference(bv)["out"][1], R.reference(bs)["out"][1]
    differ = int((ov["out"][wv] != os_["out"][ws]).sum())
    print(vec, scalar, "elements that differ between the two kernels:", differ, "of", int(wv.sum()))
    record(f"twins:{vec}:{scalar}", {"differing": differ, "elements": int(wv.sum()), "failed": fails})
    if bv.case.op == "transpose":
        assert differ == 0
    assert not fails, "\n  ".join(fails)


REFUSALS = [
    ("mp_bf16_ws4_n1_C256", {"ws": 3}), ("mp_f32_ws4_n3_C257", {"ws": 3}),
    ("ln_bf16_C1152_ldo1152_r17", {"C": 1153}), ("ln_bf16_C1152_ldo1152_r17", {"ldo": 1153}),
    ("ln_f32_C1152", {"C": 1153}), ("ln_f32_C1152", {"ldo": 1153}),
    ("im_bf16_S8_k7_ld64_rowmap", {"ld": 146}), ("im_f32_S8_k7_ld64_rowmap", {"ld": 146}),
    ("up_bf16_H6_C300", {"H2": 5}), ("up_f32_H6_C300", {"H2": 5}),                       # an odd grid: y / 2 would reach a top row that does not exist
    ("ga_bf16_n5_H64", {"H": 60}), ("ga_f32_n5_H72", {"H": 68}),                         # H % 8: the last columns would be dropped
]


@pytest.mark.parametrize("name,change", REFUSALS, ids=lambda x: x if isinstance(x, str) else "_".join(f"{k}{v}" for k, v in x.items()))
def test_launcher_refuses_before_any_launch(L, name, change):
    """criterion 8: decided on the host -- -22, nothing launched, the sentinel everywhere.  Every pointer and every other argument is the
    valid launch of the table's case (checked against the preconditions before the one argument is replaced)."""
    b = R.build(R.BY_NAME[name])
    rc, outs = launch(L, b, refuse=change)
    assert rc == -22, rc
    for n, o in outs.items():
        assert torch.equal(o, b.outs[n].init), n


@pytest.mark.parametrize("name,change", [("ln_bf16_C144_ldo192_r9", {"rows": 0}), ("ln_f32_C64", {"rows": 0}), ("ew_bf16_mode0_15x17", {"rows": 0}),
                                         ("ew_f32_mode3_15x17", {"rows": 0}), ("ga_bf16_n5_H64", {"n": 0})], ids=lambda x: x if isinstance(x, str) else "")
def test_nothing_to_do_is_not_an_error(L, name, change):
    b = R.build(R.BY_NAME[name])
    rc, outs = launch(L, b, refuse=change)
    assert rc == 0, rc
    for n, o in outs.items():
        assert torch.equal(o, b.outs[n].init), n
