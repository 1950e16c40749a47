"""CPU tests of the token log-probs: the float64 reference pinned to torch, the tie rule, the float32 restatement of the kernels' chunked sum
inside the bound the kernels are held to, the C ABI's three entry points in header / export map / ctypes table, the strategy's refusals by
name and the request's default."""
import fnmatch
import os
import re

import numpy as np
import pytest
import torch

from tests import logprob_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_logprobs", "sr_rows_read_logprobs", "sr_op_token_logprobs")


def test_reference_is_torch_log_softmax_and_topk():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((6, 5000)) * 4).astype(np.float32)
    x[2, rng.random(5000) < 0.3] = -np.inf
    tok = rng.integers(0, 5000, 6)
    tok[2] = int(np.argmax(x[2]))
    ref = R.token_logprobs(x, tok, 8)
    ls = torch.log_softmax(torch.from_numpy(x).double(), dim=-1)
    assert np.abs(ref["lp"] - ls[torch.arange(6), torch.from_numpy(tok)].numpy()).max() <= 1e-12
    tv, ti = torch.topk(ls, 8, dim=-1)
    assert np.array_equal(ref["top_ids"], ti.numpy())          # (no ties in these rows)
    assert np.abs(ref["top_lp"] - tv.numpy()).max() <= 1e-12
    assert np.abs(ref["lse"] - torch.logsumexp(torch.from_numpy(x).double(), dim=-1).numpy()).max() <= 1e-12
    greedy = R.token_logprobs(x, None, 1)
    assert np.array_equal(greedy["tok"], ti[:, 0].numpy()) and np.array_equal(greedy["lp"], greedy["top_lp"][:, 0])


def test_tie_rule_lowest_id_first():
    x = np.full((3, 40), -1.0, dtype=np.float32)
    x[0, [31, 7, 19]] = 2.0
    x[1, :] = 0.5                                      # a constant row: ids 0 .. N-1
    x[2, [39, 38]] = 3.0
    x[2, [5, 2]] = 1.0
    ref = R.token_logprobs(x, None, 4)
    ties = np.round(np.random.default_rng(4).standard_normal((5, 300)) * 2).astype(np.float32)      # many repeated values
    assert np.array_equal(R.top_n(ties, 8), np.argsort(-ties.astype(np.float64), axis=-1, kind="stable")[:, :8])
    assert ref["tok"].tolist() == [7, 0, 38]
    assert ref["top_ids"].tolist() == [[7, 19, 31, 0], [0, 1, 2, 3], [38, 39, 2, 5]]
    assert abs(ref["lp"][1] + np.log(40)) <= 1e-12


@pytest.mark.parametrize("V", [16, 4095, 4096, 4097, 151936])
def test_restatement_stays_inside_the_bound(V):
    """the float32 restatement of the chunked sum against float64 over the op table's rows: inside the bound the kernels are held to"""
    x, kinds = R.op_rows(V, len(R.KINDS), seed=V)
    rng = np.random.default_rng(1)
    worst = 0.0
    for i, kind in enumerate(kinds):
        fin = np.flatnonzero(np.isfinite(x[i]))
        for tok in (int(R.top_n(x[i:i + 1], 1)[0, 0]), int(rng.choice(fin))):
            ref = R.token_logprobs(x[i:i + 1], [tok], 0)
            got = float(R.chunked_f32(x[i], tok))
            b = float(R.bound(float(x[i, tok]), ref["lse"][0]))
            err = abs(got - float(ref["lp"][0]))
            assert err <= b, (V, kind, tok, got, float(ref["lp"][0]), b)
            worst = max(worst, err / b)
        if kind == "one_finite":
            assert float(R.chunked_f32(x[i], int(fin[0]))) == 0.0
    assert worst <= 0.5, worst          # (the bound leaves room: the restatement itself uses no more than half of it)


def test_abi_names_in_header_export_map_and_signatures():
    from socioreasoner_amd import lib
    header = open(os.path.join(ROOT, "include", "socior.h")).read()
    emap = open(os.path.join(ROOT, "socioreasoner_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", emap)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert name in lib.SIGNATURES
    assert len(lib.SIGNATURES["sr_op_token_logprobs"][1]) == 12 and len(lib.SIGNATURES["sr_rows_read_logprobs"][1]) == 7
    assert "sr_rows_read_logprobs" in lib.HELD
    # the header carries the contract
    for phrase in ("x[tok] - logsumexp(x)", "sr_decode_beam", "sr_decode_step", "top_ids[0] == tok"):
        assert phrase in header, phrase


def test_strategy_refuses_by_name():
    from roll.distributed.strategy.mi355x_strategy import check_logprobs_config
    base = dict(max_new_tokens=8, temperature=1.0, top_k=50, top_p=1.0)
    assert check_logprobs_config(base) is None and check_logprobs_config(dict(base, logprobs=None)) is None
    assert check_logprobs_config(dict(base, logprobs=0)) == 0 and check_logprobs_config(dict(base, logprobs=8)) == 8
    with pytest.raises(ValueError, match="logprobs=9"):
        check_logprobs_config(dict(base, logprobs=9))
    with pytest.raises(ValueError, match="logprobs=-1"):
        check_logprobs_config(dict(base, logprobs=-1))
    with pytest.raises(NotImplementedError, match="logprobs=2 together with num_beams=4"):
        check_logprobs_config(dict(base, logprobs=2, num_beams=4))
    with pytest.raises(NotImplementedError, match="logprobs=0 together with top_k=2000"):
        check_logprobs_config(dict(base, logprobs=0, top_k=2000))
    assert check_logprobs_config(dict(base, logprobs=1, top_k=2000, temperature=0.0)) == 1      # greedy: no host-side draw


def test_request_default_and_submit_range():
    from socioreasoner_amd.serving import Request
    r = Request(ids=np.zeros(3, dtype=np.int64), pos3=np.zeros((3, 3), dtype=np.int64), max_new=4)
    assert r.logprobs is None and r.out_logprobs is None
    # submit refuses what is not an integer in 0..8, and raises the engine's N only upwards
    from types import SimpleNamespace
    from socioreasoner_amd.serving import ContinuousBatcher
    calls = []
    cb = ContinuousBatcher.__new__(ContinuousBatcher)
    cb.engine = SimpleNamespace(cfg=SimpleNamespace(max_prefill_tokens=64, max_patches=64, max_ctx=64, max_batch=4), logprobs=calls.append)
    cb.pending = []
    mk = lambda lp: Request(ids=np.zeros(3, dtype=np.int64), pos3=np.zeros((3, 3), dtype=np.int64), max_new=4, logprobs=lp)
    for bad in (-1, 9, True, 2.7, "3"):
        with pytest.raises(ValueError, match="logprobs"):
            cb.submit(mk(bad))
    assert not calls and not cb.pending
    for lp in (None, 2, 0, 2, 8, np.int64(3)):
        cb.submit(mk(lp))
    assert calls == [2, 8] and len(cb.pending) == 6
    cb.overlap = False
    cb._hand_back()
    assert calls == [2, 8, None] and cb._lp is None
