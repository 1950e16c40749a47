"""Every bf16 prefill attention kernel path behind ``sr_op_attention`` against float64, op by op (socioreasoner_amd/csrc/attention.hip:
k_attn_prefill<16|32|80|128>, k_attn_fewq<16,16>, k_attn_prefill2<128,causal> / <80,full>).

Every call goes through ``lib.load().sr_op_attention``; the inputs, the case table and the reference are tests/attention_ref.py (pinned on
the CPU by tests/test_host_attention_ref.py, which also checks every launch made here against the contract written in include/socior.h
before a GPU sees it).  Per case:

  1. against ``attention_eager`` (HF eager's rounding points, float64-accumulated): ``assert_bf16_close(got, want, 2, 0.02)``, the bound of
     the decode attention (test_gpu_parity.py test_decode_attention_against_oracle_math) for the same chain of rounding points;
  2. against ``attention_exact`` (float64, no rounding): the kernel is no farther from exact arithmetic than the eager reference is,
     rms <= 1.5 x and max <= 2.0 x the reference's own error (the form and factors of test_gpu_round3.py's oracle criterion) -- the only
     numeric criterion of the stress rows;
  3. exact facts on bit patterns: a causal sequence's first query and every query of a 1-key sequence return that key's V row; an output
     buffer pre-filled with a sentinel keeps it everywhere the reference writes nothing (uncovered rows, rows past q_len of a partial
     tile, the columns of a wider out_stride) and nowhere else;
  4. NaN / inf / max-finite patterns in the K rows and V^T columns past a sequence's end (finite +-3e4 in the V^T tails of a v2_ok
     launch, whose contract says finite) leave every output bit unchanged;
  5. a v2_ok row equals, bit for bit, the same inputs launched with v2_ok 0 (items re-cut to 64 queries for the ViT shape, which
     k_attn_prefill would otherwise refuse with -22 -- so rc 0 at q_tile 128 already proves k_attn_prefill2 took it) and with
     SR_ATTN_VASM=0: the op-level form of the engine-level bit-identity tests.

k_attn_win64<80> cannot be reached through this entry point (sr_op_attention leaves AttnArgs.win64 zero).  It is covered transitively:
the row ``full_hd80_37_windows_of_64`` holds k_attn_prefill<80,false> to float64 on exactly the shape k_attn_win64 serves, and
test_gpu_round3.py test_window_attention_without_lds_equals_the_staged_kernel_bit_for_bit holds k_attn_win64 bit-identical to it.

The measured figures of every case are printed and, when SR_ATTN_PARITY_JSON names a file, collected there (the run recorded in
profiles/attention_ops_parity.json).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import attention_ref as AR
from tests.util import bf16_compare, switch

pytestmark = pytest.mark.gpu
SENTINEL = 0x7fc1        # a quiet-NaN bf16 pattern no kernel produces from finite inputs


@pytest.fixture(scope="module")
def L():
    from socioreasoner_amd import lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib.load()


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


_KEEP = []


def D(t):
    """host tensor -> device tensor that stays alive until the test module ends (as in test_gpu_parity.py)"""
    d = t.cuda()
    _KEEP.append(d)
    if len(_KEEP) > 64:
        torch.cuda.synchronize()
        del _KEEP[:32]
    return d


def record(name, payload):
    path = os.environ.get("SR_ATTN_PARITY_JSON")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    cur = json.load(open(path)) if os.path.exists(path) else {}
    cur[name] = payload
    json.dump(cur, open(path, "w"), indent=1, sort_keys=True)


def launch(L, b, v2_ok, n_work=None, head_dim=None, q_tile=None, causal=None):
    """one sr_op_attention launch into a sentinel-filled output; returns (rc, output bit patterns on the host as int16 [rows, out_stride]).
    The launch's buffers and work items are checked against the kernels' preconditions on the host first."""
    c = b.case
    AR.check_preconditions(b, v2_ok)
    out = torch.full((b.out_rows, b.out_stride), SENTINEL, dtype=torch.int16, device="cuda")
    work = D(torch.from_numpy(b.work_array().view(np.uint8).copy()))
    rc = L.sr_op_attention(P(D(b.q)), b.q_stride, P(D(b.k)), b.k_stride, b.k_head_stride, P(D(b.vt)), b.vt_stride, b.vt_head_stride,
                           P(out), b.out_stride, P(work), len(b.work) if n_work is None else n_work, c.heads, c.group, b.scale,
                           int(c.causal if causal is None else causal), c.hd if head_dim is None else head_dim,
                           b.q_tile if q_tile is None else q_tile, v2_ok, sp())
    torch.cuda.synchronize()
    return rc, out.cpu()


def values(bits):
    return bits.view(torch.bfloat16).double()


def where(b, r, col):
    """work item, head, query position, channel and key tiles of output element (r, col): the coordinates a kernel bug shows up in"""
    c = b.case
    for it in b.work:
        q_row0, seq_len, q_off, k_row0, vt_off, q_len = it
        nq = min(b.q_tile, (q_len or seq_len) - q_off)
        if q_row0 <= r < q_row0 + nq:
            qpos = q_off + r - q_row0
            tiles = (seq_len + AR.KT - 1) // AR.KT
            last = min(qpos // AR.KT, tiles - 1) if c.causal else tiles - 1
            return (f"row {r} col {col}: work item {it} (index {b.work.index(it)}), head {col // c.hd}, kv head {col // c.hd // c.group}, "
                    f"query position {qpos}, channel {col % c.hd}, last visible key tile {last} of {tiles} ({seq_len} keys)")
    return f"row {r} col {col}: no work item covers it"


def worst(b, diff, mask):
    d = torch.where(mask, diff, torch.zeros_like(diff))
    i = int(d.argmax())
    return where(b, i // b.out_stride, i % b.out_stride)


def v_row_bits(b, si, h):
    c = b.case
    return torch.as_strided(b.vt.view(torch.int16), (c.hd,), (b.vt_stride,), si["vt_off"] + (h // c.group) * b.vt_head_stride)


def containment(b, bits, written, fails, what=""):
    sent = bits == SENTINEL
    if not bool(sent[~written].all()):
        bad = (~sent & ~written).nonzero()
        r, col = (int(x) for x in bad[0])
        fails.append(f"{what}write outside the work items: {len(bad)} elements, first {where(b, r, col)}")
    if bool(sent[written].any()):
        bad = (sent & written).nonzero()
        r, col = (int(x) for x in bad[0])
        fails.append(f"{what}{len(bad)} elements the work items define were not written, first {where(b, r, col)}")


def rows_equal_v(b, bits, si, rows, fails, what):
    c = b.case
    for h in range(c.heads):
        want = v_row_bits(b, si, h)
        got = bits[si["q_row0"] + rows[0]: si["q_row0"] + rows[-1] + 1, h * c.hd: (h + 1) * c.hd]
        if not torch.equal(got, want.expand_as(got)):
            bad = (got != want.expand_as(got)).nonzero()[0]
            fails.append(f"{what}: {where(b, si['q_row0'] + rows[0] + int(bad[0]), h * c.hd + int(bad[1]))} is not the V row")
            return


def err(a, ref):
    d = (a - ref).flatten()
    return {"rms": float(d.pow(2).mean().sqrt()), "max": float(d.abs().max())}


@pytest.mark.parametrize("case", AR.CASES, ids=lambda c: c.name)
def test_attention_kernel_against_float64(L, monkeypatch, case):
    """(module docstring) criteria 1-5 for one row of the case table; every failed criterion is reported, with the worst element's work
    item, head, query position and key tile."""
    b = AR.build(case)
    rc, bits = launch(L, b, case.v2_ok)
    assert rc == 0, rc
    eager, written = AR.attention_eager(*b.ref_args())
    exact, w2 = AR.attention_exact(*b.ref_args())
    assert torch.equal(written, w2)
    fails, res = [], {"kernel": case.kernel, "stress": case.stress, "elements": int(written.sum())}
    # ---- 3. containment and exact facts
    containment(b, bits, written, fails)
    got = values(bits)
    g, e, x = got[written], eager[written], exact[written]
    if not bool(torch.isfinite(g).all()):
        fails.append(f"non-finite output: {worst(b, (~torch.isfinite(got)).double(), written)}")
        g = torch.nan_to_num(g, nan=1e30, posinf=1e30, neginf=-1e30)
        got = torch.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
    for si in b.seq_info:
        if si["keys"] == 1:
            rows_equal_v(b, bits, si, list(range(si["nq"])), fails, "1-key sequence")
        elif case.causal:
            rows_equal_v(b, bits, si, [0], fails, "first query of a causal sequence")
    # ---- 1. eager reference (figures always recorded; asserted for the rows outside the stress set)
    mu, frac, mad = bf16_compare(g, e)
    res["vs_eager"] = {"max_ulp": mu, "share": frac, "max_abs": mad}
    if not case.stress and not (mu <= 2 + 1e-6 and frac <= 0.02):
        fails.append(f"eager reference: max {mu:.2f} ulp, {frac:.4%} differ, max abs {mad:.3e} (bound 2 ulp, 2 %); worst abs: "
                     f"{worst(b, (got - eager).abs(), written)}")
    # ---- 2. float64
    e_ref, e_hip = err(e, x), err(g, x)
    res["vs_float64"] = {"reference": e_ref, "kernel": e_hip, "rms_ratio": e_hip["rms"] / e_ref["rms"] if e_ref["rms"] else float(e_hip["rms"] > 0),
                         "max_ratio": e_hip["max"] / e_ref["max"] if e_ref["max"] else float(e_hip["max"] > 0)}
    if not (e_hip["rms"] <= 1.5 * e_ref["rms"] and e_hip["max"] <= 2.0 * e_ref["max"]):
        fails.append(f"float64: kernel {e_hip} against the eager reference's own {e_ref} (bound 1.5 x rms, 2.0 x max); worst: "
                     f"{worst(b, (got - exact).abs(), written)}")
    # ---- 4. what lies past the end of a sequence must not leak
    gb = AR.build(case, tail="garbage")
    rc, bits_g = launch(L, gb, case.v2_ok)
    if rc != 0 or not torch.equal(bits_g, bits):
        fails.append(f"garbage past the sequences leaks (rc {rc}): {int((bits_g != bits).sum())} elements change, first "
                     f"{worst(b, (bits_g != bits).double(), torch.ones_like(written))}")
    # ---- 5. the LDS-DMA kernel and its hand-issued V^T reads against k_attn_prefill
    if case.v2_ok:
        twin = AR.build(case, q_tile=64)
        rc, bits_1 = launch(L, twin, 0)
        if rc != 0 or not torch.equal(bits_1, bits):
            fails.append(f"v2_ok 1 and v2_ok 0 differ (rc {rc}): {int((bits_1 != bits).sum())} elements, first "
                         f"{worst(b, (bits_1 != bits).double(), torch.ones_like(written))}")
        switch(monkeypatch, "SR_ATTN_VASM", 0)
        rc, bits_c = launch(L, b, 1)
        switch(monkeypatch, "SR_ATTN_VASM", None)
        if rc != 0 or not torch.equal(bits_c, bits):
            fails.append(f"SR_ATTN_VASM=0 differs (rc {rc}): {int((bits_c != bits).sum())} elements, first "
                         f"{worst(b, (bits_c != bits).double(), torch.ones_like(written))}")
    res["failed"] = fails
    print(case.name, json.dumps(res))
    record(case.name, res)
    assert not fails, case.name + ":\n  " + "\n  ".join(fails)


@pytest.mark.parametrize("case", AR.UNIFORM_CASES, ids=lambda c: c.name)
def test_uniform_softmax_returns_the_v_row_bit_for_bit(L, case):
    """q = 0 makes every score exactly 0; with 64 / 1024 / 4096 keys (no partial tile, non-causal) every P is exactly 1 / n, and with
    identical V rows every product and every partial sum m * v / n (m <= 4096, v an 8-bit mantissa) is exact in float32 in any order:
    the output is the V row, on k_attn_prefill, k_attn_fewq (partials of 1, 16 and 64 tiles over 16 waves) and k_attn_prefill2."""
    b = AR.build(case, uniform=True)
    variants = [("", b, case.v2_ok)] + ([("v2_ok 0: ", AR.build(case, uniform=True, q_tile=64), 0)] if case.v2_ok else [])
    fails = []
    for what, bb, v2 in variants:
        rc, bits = launch(L, bb, v2)
        assert rc == 0, rc
        written = bb.written_map()
        containment(bb, bits, written, fails, what)
        for si in bb.seq_info:
            rows_equal_v(bb, bits, si, list(range(si["nq"])), fails, f"{what}{si['keys']} keys")
    assert not fails, "\n  ".join(fails)


@pytest.mark.parametrize("hd,q_tile,causal", [(32, 16, 0), (16, 16, 1), (80, 64, 1), (64, 64, 0), (128, 32, 1)])
def test_launcher_refuses_unsupported_shapes_before_any_launch(L, hd, q_tile, causal):
    """launch_attn_prefill decides these on the host: -22, nothing launched, the output untouched.  (Only refusals of well-formed
    arguments are tested: every pointer, stride and work item below is valid for a kernel of that head_dim.)"""
    b = AR.build(AR.Case("refused", "-", hd, bool(causal), q_tile, 0, 4, 1, ((40, 0), (17, 0)), seed=3000 + hd))
    rc, bits = launch(L, b, 0)
    assert rc == -22, rc
    assert bool((bits == SENTINEL).all())


def test_no_work_items_is_not_an_error(L):
    b = AR.build(AR.Case("empty", "-", 80, False, 64, 0, 4, 1, ((40, 0),), seed=3100))
    rc, bits = launch(L, b, 0, n_work=0)
    assert rc == 0, rc
    assert bool((bits == SENTINEL).all())
