"""GPU tests of the token log-probs (sr_logprobs): the kernels alone against the float64 definition, the static greedy and sampled decodes,
the continuous batcher (plain and overlapped, both CU-hint forms) against teacher-forced float64 log-probs, and the strategy layers.
SR_LOGPROBS_PROFILE=<path> writes the measured maxima as JSON when the module ends."""
import ctypes as C
import json
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from tests import logprob_ref as R

pytestmark = pytest.mark.gpu

MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("SR_LOGPROBS_PROFILE")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _note(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(value))


def _sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _geom(size):
    from socioreasoner_amd.config import geometry_3b, geometry_tiny
    if size == "tiny":
        return geometry_tiny(), 2000
    g = geometry_3b()
    return replace(g, text=replace(g.text, num_hidden_layers=4), vision=replace(g.vision, depth=2, fullatt_block_indexes=(1,))), 150000


def _prompts(rng, n, lo=5, hi=40, vocab=2000):
    ids = [rng.integers(0, vocab, int(rng.integers(lo, hi))).astype(np.int64) for _ in range(n)]
    pos = [np.tile(np.arange(len(x)), (3, 1)).astype(np.int64) for x in ids]
    return ids, pos


def _engine(size, MB, max_new, max_ctx=128, kv_slots=0):
    from socioreasoner_amd.engine import Engine
    geom, vocab = _geom(size)
    e = Engine(geom, max_patches=64, max_prefill_tokens=4096, max_batch=MB, max_ctx=max_ctx, max_new_tokens=max_new, kv_slots=kv_slots)
    e.load_synthetic_weights(seed=0)
    return e, vocab


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
GUARD = 64
S_F, S_I = 12345.0, -7777


def _op(lib, Lb, x_dev, ld, rows, V, tokens, row_map, n, logits_ptr=None):
    """one sr_op_token_logprobs call into sentinel-filled outputs with guard regions -> (lp, tok, top_ids, top_lp) on the host; asserts the guards"""
    lp = torch.full((rows + 2 * GUARD,), S_F, dtype=torch.float32, device="cuda")
    tk = torch.full((rows + 2 * GUARD,), S_I, dtype=torch.int32, device="cuda")
    ti = torch.full((rows * 8 + 2 * GUARD,), S_I, dtype=torch.int32, device="cuda")
    tl = torch.full((rows * 8 + 2 * GUARD,), S_F, dtype=torch.float32, device="cuda")
    tok_d = None if tokens is None else torch.as_tensor(tokens, dtype=torch.int64, device="cuda")
    map_d = None if row_map is None else torch.as_tensor(row_map, dtype=torch.int32, device="cuda")
    lib.check(Lb.sr_op_token_logprobs(logits_ptr if logits_ptr is not None else x_dev.data_ptr(), ld, rows, V,
                                      None if tok_d is None else tok_d.data_ptr(), None if map_d is None else map_d.data_ptr(), n,
                                      lp.data_ptr() + 4 * GUARD, tk.data_ptr() + 4 * GUARD, ti.data_ptr() + 4 * GUARD, tl.data_ptr() + 4 * GUARD, _sp()),
              None, "sr_op_token_logprobs")
    torch.cuda.synchronize()
    for t, s in ((lp, S_F), (tk, S_I), (ti, S_I), (tl, S_F)):
        assert (t[:GUARD] == s).all() and (t[-GUARD:] == s).all(), "guard region written"
    return (lp[GUARD:-GUARD].cpu().numpy(), tk[GUARD:-GUARD].cpu().numpy().astype(np.int64),
            ti[GUARD:-GUARD].cpu().numpy().reshape(rows, 8).astype(np.int64), tl[GUARD:-GUARD].cpu().numpy().reshape(rows, 8))


def _check_records(got, x, tokens, n, key, ls=None):
    """device records against the float64 definition on the float32 rows x: ids and tokens exact, lp / top_lp inside the bound"""
    lp, tk, ti, tl = got
    ref = R.token_logprobs(x, tokens, n, ls)
    rows = x.shape[0]
    assert np.array_equal(tk, ref["tok"])
    xt = x[np.arange(rows), ref["tok"]].astype(np.float64)
    fin = np.isfinite(ref["lp"])
    assert np.array_equal(lp[~fin], ref["lp"][~fin].astype(np.float32))          # (-inf stays -inf)
    b = R.bound(np.where(fin, xt, 0.0), ref["lse"])
    err = np.abs(lp.astype(np.float64) - ref["lp"])[fin] / b[fin]
    print(f"{key}: max |lp - lp64| / bound = {err.max() if err.size else 0:.4f}")
    if err.size:
        _note(key + " lp/bound", err.max())
        assert err.max() <= 1.0, (key, err.max())
    assert np.array_equal(ti[:, :n], ref["top_ids"]), key
    assert (ti[:, n:] == -1).all() and (tl[:, n:] == 0).all()
    if n:
        xi = np.take_along_axis(x, ref["top_ids"], axis=-1).astype(np.float64)
        fin = np.isfinite(ref["top_lp"])
        assert np.array_equal(tl[:, :n][~fin], ref["top_lp"][~fin].astype(np.float32))
        bt = R.bound(np.where(fin, xi, 0.0), ref["lse"][:, None])
        with np.errstate(invalid="ignore"):          # (-inf entries: compared exactly above, masked out here)
            err = (np.abs(tl[:, :n].astype(np.float64) - ref["top_lp"]) / bt)[fin]
        print(f"{key}: max |top_lp - top_lp64| / bound = {err.max():.4f}")
        _note(key + " top_lp/bound", err.max())
        assert err.max() <= 1.0, (key, err.max())
    return ref


@pytest.mark.parametrize("rows", [1, 3, 32, 128])
@pytest.mark.parametrize("V", [16, 4095, 4096, 4097, 151936])
def test_op_token_logprobs(V, rows):
    """sr_op_token_logprobs over the op table (every row kind of logprob_ref.op_rows), ld == V and ld > V with NaN in the pad columns, tokens
    given and null, identity and repeating row maps, N in 0 / 1 / 8: ids and tokens exact, lp and top_lp within
    8 x 2^-23 x max(8, |x_tok|, |lse64|) of float64, nothing written outside the outputs; special rows hold their exact values."""
    from socioreasoner_amd import lib
    Lb = lib.load()
    x, kinds = R.op_rows(V, rows, seed=1000 + V + rows)
    rng = np.random.default_rng(V * 131 + rows)
    pad = 0 if rows in (1, 32) else 5
    ld = V + pad
    buf = torch.full((rows, ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(x).cuda()
    tokens = np.array([int(rng.choice(np.flatnonzero(np.isfinite(x[i])))) if i % 3 else int(rng.integers(0, V)) for i in range(rows)])
    row_map = rng.integers(0, rows, rows)
    if rows >= 3:
        row_map[1] = row_map[0]          # (a repeat for certain)
    ls = R.log_softmax64(x)          # (the reference, computed once)
    for n in (0, 1, 8):
        key = f"op V={V}"
        g_arg = _check_records(_op(lib, Lb, buf, ld, rows, V, None, None, n), x, None, n, key, ls)
        _check_records(_op(lib, Lb, buf, ld, rows, V, tokens, None, n), x, tokens, n, key, ls)
        _check_records(_op(lib, Lb, buf, ld, rows, V, tokens, row_map, n), x[row_map], tokens, n, key, ls[row_map])
        lp, tk, ti, tl = _op(lib, Lb, buf, ld, rows, V, None, row_map, n)
        if n:      # greedy identity, bit for bit
            assert np.array_equal(ti[:, 0], tk) and np.array_equal(tl[:, 0], lp)
        # the special rows
        lp, tk, ti, tl = _op(lib, Lb, buf, ld, rows, V, None, None, n)
        for i, kind in enumerate(kinds):
            if kind == "constant":
                assert tk[i] == 0 and ti[i, :n].tolist() == list(range(n))
                assert abs(float(lp[i]) + np.log(V)) <= float(R.bound(float(x[i, 0]), g_arg["lse"][i]))
            if kind == "one_finite":
                assert float(lp[i]) == 0.0 and tk[i] == int(np.flatnonzero(np.isfinite(x[i]))[0])
            if kind == "dup_max":
                assert tk[i] == int(np.flatnonzero(x[i] == x[i].max())[0])


def test_op_row_independence():
    """a row launched alone and among 127 others gives the same bits (N = 8, tokens given and arg-max)"""
    from socioreasoner_amd import lib
    Lb = lib.load()
    V, rows = 151936, 128
    x, _ = R.op_rows(V, rows, seed=77)
    buf = torch.from_numpy(x).cuda()
    tokens = np.random.default_rng(3).integers(0, V, rows)
    for toks in (None, tokens):
        full = _op(lib, Lb, buf, V, rows, V, toks, None, 8)
        for i in (0, 5, 77, 127):
            one = _op(lib, Lb, buf, V, 1, V, None if toks is None else toks[i:i + 1], None, 8, logits_ptr=buf.data_ptr() + 4 * V * i)
            for a, b in zip(full, one):
                assert np.array_equal(a[i:i + 1].view(np.int32) if a.dtype == np.float32 else a[i:i + 1],
                                      b.view(np.int32) if b.dtype == np.float32 else b), i


def test_op_optional_outputs_null():
    """tok_out and the two top arrays are optional (the engine passes no tok_out): lp alone equals the full call's bit for bit"""
    from socioreasoner_amd import lib
    Lb = lib.load()
    V, rows = 4097, 32
    x, _ = R.op_rows(V, rows, seed=5)
    buf = torch.from_numpy(x).cuda()
    for n in (0, 8):
        full = _op(lib, Lb, buf, V, rows, V, None, None, n)
        lp = torch.full((rows + 2 * GUARD,), S_F, dtype=torch.float32, device="cuda")
        ti = torch.full((rows * 8,), S_I, dtype=torch.int32, device="cuda")
        tl = torch.full((rows * 8,), S_F, dtype=torch.float32, device="cuda")
        for tops in (False, True):
            lib.check(Lb.sr_op_token_logprobs(buf.data_ptr(), V, rows, V, None, None, n, lp.data_ptr() + 4 * GUARD, None, ti.data_ptr() if tops else None,
                                              tl.data_ptr() if tops else None, _sp()), None, "sr_op_token_logprobs")
            torch.cuda.synchronize()
            assert (lp[:GUARD] == S_F).all() and (lp[-GUARD:] == S_F).all()
            assert np.array_equal(lp[GUARD:-GUARD].cpu().numpy().view(np.int32), full[0].view(np.int32))
        assert np.array_equal(ti.cpu().numpy().reshape(rows, 8), full[2]) and np.array_equal(tl.cpu().numpy().reshape(rows, 8).view(np.int32), full[3].view(np.int32))
    # one top array without the other is refused
    assert Lb.sr_op_token_logprobs(buf.data_ptr(), V, rows, V, None, None, 1, lp.data_ptr(), None, ti.data_ptr(), None, _sp()) == -22


def test_op_refusals():
    from socioreasoner_amd import lib
    Lb = lib.load()
    x = torch.zeros(2, 32, dtype=torch.float32, device="cuda")
    lp = torch.zeros(2, dtype=torch.float32, device="cuda")
    for n in (-1, 9):
        assert Lb.sr_op_token_logprobs(x.data_ptr(), 32, 2, 32, None, None, n, lp.data_ptr(), None, None, None, _sp()) == -22
        assert f"top_n {n}" in Lb.sr_last_error(None).decode()
    e, _ = _engine("tiny", 2, 4)
    for n in (-2, 9):
        with pytest.raises(lib.SocioRError, match=f"top_n {n}"):
            e.logprobs(n)
    e.close()


# ------------------------------------------------------------------------------------------------ 2. static greedy
def _trace_check(rec, tr, toks, lens, n, key, chosen=None):
    """records [B, max_new(, 8)] against the float64 definition on the traced logits tr [max_new, B, V]; positions past a row's length hold
    (0, -1, 0).  chosen: the logged tokens where they are not the arg-max"""
    lp, ids, tlp = (t.cpu().numpy() for t in rec)
    B, max_new = lp.shape
    x_all = tr.cpu().numpy()
    for b in range(B):
        L = int(lens[b])
        x = x_all[:L, b]
        got = (lp[b, :L], np.asarray(toks[b][:L], dtype=np.int64), ids[b, :L].astype(np.int64), tlp[b, :L])
        _check_records(got, x, None if chosen is None else np.asarray(chosen[b][:L]), n, key)
        assert (lp[b, L:] == 0).all() and (ids[b, L:] == -1).all() and (tlp[b, L:] == 0).all(), "pads must read (0, -1, 0)"


@pytest.mark.parametrize("size,B", [("tiny", 1), ("tiny", 17), ("tiny", 32), ("3b", 1), ("3b", 17), ("3b", 32)])
def test_static_greedy(size, B):
    """sr_decode under the switch: the tokens of the run without it; lp and top-8 within the op bound of the float64 definition on the traced
    logits; top_ids[0] == tok and top_lp[0] == lp bit for bit; a graph replay gives the eager records bit for bit; rows that met eos early
    pad with (0, -1, 0)."""
    max_new = 12
    e, vocab = _engine(size, 32, max_new)
    ids, pos = _prompts(np.random.default_rng(40 + B), B, vocab=vocab)
    pad = vocab - 1
    e.prefill(ids, pos)
    free = e.decode(max_new, eos=[], pad_id=pad).cpu()
    assert e.token_logprobs is None
    # eos tokens that some rows meet early: what rows 0 and B - 1 emit at position 3
    eos = sorted({int(free[0, 3]), int(free[B - 1, 3])})
    e.prefill(ids, pos)
    base = e.decode(max_new, eos=eos, pad_id=pad).cpu()
    lens = [next((t + 1 for t in range(max_new) if int(base[b, t]) in eos), max_new) for b in range(B)]
    assert min(lens) < max_new
    e.logprobs(8)
    e.prefill(ids, pos)
    toks, tr = e.decode(max_new, eos=eos, pad_id=pad, trace=True, use_graph=False)
    assert torch.equal(toks.cpu(), base)
    eager = e.token_logprobs
    _trace_check(eager, tr, toks.cpu().tolist(), lens, 8, f"static greedy {size}")
    lp, ti, tl = eager
    for b in range(B):
        L = lens[b]
        assert torch.equal(ti[b, :L, 0].cpu(), toks[b, :L].cpu()) and torch.equal(tl[b, :L, 0], lp[b, :L])
    e.prefill(ids, pos)
    toks_g = e.decode(max_new, eos=eos, pad_id=pad)
    assert torch.equal(toks_g.cpu(), base)
    for a, b_ in zip(eager, e.token_logprobs):
        assert torch.equal(a, b_), "graph replay differs from the eager launches"
    e.logprobs(None)
    e.prefill(ids, pos)
    assert torch.equal(e.decode(max_new, eos=eos, pad_id=pad).cpu(), base) and e.token_logprobs is None
    e.close()


# ------------------------------------------------------------------------------------------------ teacher forcing (3, 4)
def _teacher(e, ids, pos, seqs, max_new, pad, rows=None):
    """float64 log_softmax [max_new, n, V] of the given sequences (token lists, padded here) teacher-forced through plain decode from a fresh
    prefill, in groups of `rows` rows (default: max_batch)"""
    MB = rows or e.cfg.max_batch
    out = []
    for g0 in range(0, len(seqs), MB):
        grp = list(range(g0, min(g0 + MB, len(seqs))))
        fill = grp + [grp[-1]] * (MB - len(grp))                      # always the same row count
        forced = torch.full((MB, max_new), pad, dtype=torch.int32)
        for r, k in enumerate(fill):
            forced[r, :len(seqs[k])] = torch.tensor(seqs[k], dtype=torch.int32)
        e.prefill([ids[k] for k in fill], [pos[k] for k in fill])
        _, lg = e.decode(max_new, eos=[], pad_id=pad, trace=True, forced=forced, use_graph=False)
        out.append(torch.log_softmax(lg[:, :len(grp)].double(), dim=-1).cpu())
    return torch.cat(out, dim=1)


def _teacher_check(ls, k, toks, rec, n, key):
    """sequence k's records against the teacher-forced float64 log-probs ls [max_new, n_seq, V]: lp within 1e-4 x max(1, |lp|); top ids equal
    wherever the gap between the reference's adjacent log-probs exceeds that bound"""
    worst = 0.0
    assert len(rec["logprobs"]) == len(toks) and len(rec["top"]) == len(toks)
    for t, tok in enumerate(toks):
        want = float(ls[t, k, tok])
        tol = 1e-4 * max(1.0, abs(want))
        err = abs(rec["logprobs"][t] - want)
        worst = max(worst, err / tol)
        assert err <= tol, (key, k, t, rec["logprobs"][t], want)
        assert len(rec["top"][t]) == n
        if n:
            tv, ti = torch.topk(ls[t, k], n + 1)
            for j, (i_got, v_got) in enumerate(rec["top"][t]):
                tol_j = 1e-4 * max(1.0, abs(float(tv[j])))
                clear = (j == 0 or float(tv[j - 1] - tv[j]) > tol_j) and float(tv[j] - tv[j + 1]) > tol_j
                if clear:
                    assert i_got == int(ti[j]), (key, k, t, j)
                    assert abs(v_got - float(tv[j])) <= tol_j
    _note(key + " lp/(1e-4 max(1,|lp|))", worst)
    return worst


def _as_rec(rec, b, L, n):
    lp, ids, tlp = rec
    return {"logprobs": lp[b, :L].tolist(), "top": [list(zip(ids[b, t, :n].tolist(), tlp[b, t, :n].tolist())) for t in range(L)]}


@pytest.mark.parametrize("size,B,rp", [("tiny", 17, 1.0), ("3b", 32, 1.0), ("tiny", 32, 1.3)])
def test_static_sampled(size, B, rp):
    """sr_decode_sample under the switch (N = 2): the tokens of the run without it; every token's lp within 1e-4 x max(1, |lp|) of the
    float64 log-prob of the sequence teacher-forced from a fresh prefill; graph replay == eager launches bit for bit."""
    max_new = 10
    e, vocab = _engine(size, 32, max_new)
    ids, pos = _prompts(np.random.default_rng(60 + B), B, vocab=vocab)
    pad = vocab - 1
    kw = dict(temperature=1.0, top_k=50, top_p=0.9, repetition_penalty=rp, seed=5, eos=[], pad_id=pad)
    e.prefill(ids, pos)
    base = e.decode_sample(max_new, **kw).cpu()
    e.logprobs(2)
    e.prefill(ids, pos)
    toks = e.decode_sample(max_new, **kw).cpu()
    assert torch.equal(toks, base)
    rec = tuple(t.cpu() for t in e.token_logprobs)
    e.prefill(ids, pos)
    assert torch.equal(e.decode_sample(max_new, use_graph=False, **kw).cpu(), base)
    for a, b_ in zip(rec, e.token_logprobs):
        assert torch.equal(a, b_.cpu()), "eager launches differ from the graph replay"
    assert (rec[1][:, :, 2:] == -1).all() and (rec[2][:, :, 2:] == 0).all()
    e.logprobs(None)
    ls = _teacher(e, ids, pos, toks.tolist(), max_new, pad, rows=B)
    for b in range(B):
        _teacher_check(ls, b, toks[b].tolist(), _as_rec(rec, b, max_new, 2), 2, f"static sampled {size}")
    e.close()


# ------------------------------------------------------------------------------------------------ 4. the continuous batcher
def _requests(ids, pos, with_lp, max_new):
    """greedy, sampled, penalised and n = 3 fan-out requests, long ones followed by short ones (rows are re-used), some asking for log-probs
    0 / 2 / 8"""
    from socioreasoner_amd.serving import Request
    reqs = []
    for k in range(len(ids)):
        kind = k % 4
        smp = (None, {"temperature": 1.0, "top_k": 40, "top_p": 0.9, "seed": 11 + k},
               {"temperature": 0.8, "top_k": -1, "top_p": 0.95, "repetition_penalty": 1.2, "seed": 3 + k}, {"temperature": 0.9, "top_k": 20, "seed": 100 + k})[kind]
        lpn = (8, 2, None, 2, 0, None, 0, 8)[k % 8] if with_lp else None          # (the n = 3 requests, k % 4 == 3, ask 2 and 8)
        reqs.append(Request(ids=ids[k], pos3=pos[k], max_new=max_new if (k // 4) % 2 == 0 else 3 + k % 4, n=3 if kind == 3 else 1, sampling=smp,
                            logprobs=lpn))
    return reqs


def _serve(e, reqs, overlap, cus, sampling=None):
    from socioreasoner_amd.serving import ContinuousBatcher
    if cus:
        e.rows_set_cus(cus)
        e._decode_cus = cus
    cb = ContinuousBatcher(e, eos=[], pad_id=0, steps_per_poll=4, overlap=overlap, sampling=sampling)
    out = cb.run(reqs)
    e.rows_set_cus(0)
    e._decode_cus = 0
    assert cb.idle() and e.top_logprobs is None
    return out


@pytest.mark.parametrize("size,MB", [("tiny", 32), ("3b", 32), ("tiny", 64)])
def test_batcher_records(size, MB):
    """The mixed request stream through the continuous batcher, plain and overlapped, with the CU hint 0 and 160: tokens identical to the same
    run with no request asking; every returned sequence teacher-forced: lp within 1e-4 x max(1, |lp|) of float64, top-N ids equal where the
    reference's gaps exceed the bound; requests that did not ask get nothing; records bit-identical across the CU hint, and across overlap
    on / off for the greedy requests."""
    max_new = 12
    e, vocab = _engine(size, MB, max_new, kv_slots=2 * MB)
    n_req = MB + 12 if MB == 32 else MB + 8
    ids, pos = _prompts(np.random.default_rng(7 + MB), n_req, vocab=vocab)
    quiet = _serve(e, _requests(ids, pos, False, max_new), False, 0)
    runs = {}
    for overlap, cus in ((False, 0), (False, 160), (True, 0)):      # (the overlapped batcher moves the CU hint itself: 160 CUs next to an admission)
        reqs = _requests(ids, pos, True, max_new)
        out = _serve(e, reqs, overlap, cus)
        runs[(overlap, cus)] = (out, [r.out_logprobs for r in reqs])
        for r in reqs:
            assert (r.out_logprobs is None) == (r.logprobs is None)
    out0, lp0 = runs[(False, 0)]
    assert out0 == quiet, "asking for log-probs changed tokens"
    assert runs[(False, 160)] == (out0, lp0), "tokens or records depend on the CU hint"
    out_o, lp_o = runs[(True, 0)]
    assert out_o == _serve(e, _requests(ids, pos, False, max_new), True, 0), "asking for log-probs changed tokens of the overlapped run"
    for k, r in enumerate(reqs):
        if r.sampling is None:          # greedy requests: overlap on / off
            assert out_o[k] == out0[k] and lp_o[k] == lp0[k], k
    # teacher forcing of every returned sequence (plain and overlapped runs)
    pad = vocab - 1
    for name in ((False, 0), (True, 0)):
        out, lps = runs[name]
        seqs, owner = [], []
        for k, r in enumerate(reqs):
            for j, s in enumerate(out[k] if r.n > 1 else [out[k]]):
                seqs.append(s)
                owner.append((k, j))
        ls = _teacher(e, [ids[k] for k, _ in owner], [pos[k] for k, _ in owner], seqs, max_new, pad)
        for i, (k, j) in enumerate(owner):
            r = reqs[k]
            if r.logprobs is None:
                continue
            rec = lps[k][j] if r.n > 1 else lps[k]
            _teacher_check(ls, i, seqs[i], rec, r.logprobs, f"batcher {size} {MB} rows")
    e.close()


def test_batcher_shared_sampled_step():
    """a batcher whose shared configuration samples (the rows-sampled step): tokens as without the switch, records held to teacher forcing"""
    max_new = 10
    e, vocab = _engine("tiny", 8, max_new, kv_slots=16)
    ids, pos = _prompts(np.random.default_rng(91), 12, vocab=vocab)
    from socioreasoner_amd.serving import Request
    shared = {"temperature": 1.0, "top_k": 30, "top_p": 0.9, "seed": 9}
    mk = lambda lp: [Request(ids=ids[k], pos3=pos[k], max_new=max_new if k % 3 else 4, logprobs=lp if k % 2 else None) for k in range(12)]
    quiet = _serve(e, mk(None), False, 0, shared)
    reqs = mk(3)
    out = _serve(e, reqs, False, 0, shared)
    assert out == quiet
    ls = _teacher(e, ids, pos, out, max_new, vocab - 1)
    for k, r in enumerate(reqs):
        assert (r.out_logprobs is None) == (k % 2 == 0)
        if k % 2:
            _teacher_check(ls, k, out[k], r.out_logprobs, 3, "batcher shared sampled tiny")
    e.close()


def test_batcher_abort_delivers_nothing():
    from socioreasoner_amd.serving import ContinuousBatcher, Request
    e, vocab = _engine("tiny", 8, 12, kv_slots=16)
    ids, pos = _prompts(np.random.default_rng(2), 6, vocab=vocab)
    reqs = [Request(ids=ids[k], pos3=pos[k], max_new=12, logprobs=2, tag=k) for k in range(6)]
    cb = ContinuousBatcher(e, eos=[], pad_id=0, steps_per_poll=2)
    for r in reqs:
        cb.submit(r)
    got = {}
    cb.pump(lambda r, t: got.__setitem__(r.tag, t))
    cb.abort(lambda r: r.tag in (1, 4))
    while not cb.idle():
        cb.pump(lambda r, t: got.__setitem__(r.tag, t))
    cb._hand_back()
    for r in reqs:
        if r.tag in (1, 4):
            assert r.aborted and r.out_logprobs is None
        else:
            assert len(r.out_logprobs["logprobs"]) == len(got[r.tag]) == 12 and all(len(t) == 2 for t in r.out_logprobs["top"])
    e.close()


# ------------------------------------------------------------------------------------------------ 5. strategy
def _strategy(max_batch=8):
    from roll.distributed.strategy.factory import create_strategy

    class W:   # minimal worker (as tests/test_gpu_pipeline.py)
        rank, world_size = 0, 1
        pipeline_config = type("P", (), {"prompt_length": 64, "response_length": 16})()
        worker_config = type("C", (), {"strategy_args": type("S", (), {"strategy_name": "mi355x", "strategy_config": {"max_batch": max_batch, "max_ctx": 128}})(),
                                       "model_args": type("M", (), {"model_name_or_path": "synthetic:tiny"})()})()
        rank_info = type("R", (), {"local_rank": 0})()
    st = create_strategy(W())
    st.initialize(None)
    return st


def test_strategy_generate_and_server():
    """generate and start_server with and without generation_config["logprobs"]: list lengths equal the response lengths, the order follows the
    returned rows, greedy n > 1 copies like the tokens, and nothing new appears without the key."""
    from roll.distributed.scheduler.protocol import DataProto
    st = _strategy()
    rng = np.random.default_rng(8)
    P, B = 24, 3
    ids = torch.from_numpy(rng.integers(0, 2000, size=(B, P))).long()
    mk = lambda: DataProto(batch={"input_ids": ids, "attention_mask": torch.ones(B, P, dtype=torch.long)}, non_tensor_batch={}, meta_info={})
    base = dict(max_new_tokens=12, eos_token_id=[2046], pad_token_id=2045, num_beams=1)
    smp = dict(base, temperature=1.0, top_k=100, top_p=0.8, seed=4, num_return_sequences=2)
    b0 = mk()
    plain = st.generate(b0, smp)
    assert "output_logprobs" not in b0.meta_info and "output_top_logprobs" not in b0.meta_info
    for n_top in (0, 3):
        b1 = mk()
        out = st.generate(b1, dict(smp, logprobs=n_top))
        assert torch.equal(out, plain)
        lps = b1.meta_info["output_logprobs"]
        assert len(lps) == out.shape[0] == 2 * B
        assert ("output_top_logprobs" in b1.meta_info) == (n_top > 0)
        for row, lp in zip(out, lps):
            resp = row[P:].tolist()
            cut = next((j + 1 for j, t in enumerate(resp) if int(t) == 2046), len(resp))      # (a row without eos ran all max_new tokens)
            assert len(lp) == cut and all(v <= 0 for v in lp)
        if n_top:
            for row, lp, top in zip(out, lps, b1.meta_info["output_top_logprobs"]):
                assert len(top) == len(lp) and all(len(t) == n_top for t in top)
                for t, (tok, v) in enumerate(zip(row[P:].tolist(), lp)):      # a drawn token that is among the top entries carries their value
                    hit = [tv for ti, tv in top[t] if ti == int(tok)]
                    assert not hit or hit[0] == v
    assert st.engine.top_logprobs is None
    bg = mk()
    g = st.generate(bg, dict(base, temperature=0.0, num_return_sequences=2, logprobs=1))
    lg, tg = bg.meta_info["output_logprobs"], bg.meta_info["output_top_logprobs"]
    assert torch.equal(g[0::2], g[1::2]) and lg[0::2] == lg[1::2] and len(lg) == 2 * B
    for row, lp, top in zip(g, lg, tg):          # greedy: the token is the first top entry, bit for bit
        assert [t[0][0] for t in top] == row[P:P + len(lp)].tolist() and [t[0][1] for t in top] == lp
    with pytest.raises(NotImplementedError, match="num_beams"):
        st.generate(mk(), dict(base, num_beams=2, logprobs=1))

    def serve(confs):
        done = {}
        for k, gc in enumerate(confs):
            p = (0, 0, 1, 2)[k]
            st.add_request("ADD", DataProto(batch={"input_ids": ids[p:p + 1], "attention_mask": torch.ones(1, P, dtype=torch.long)}, non_tensor_batch={},
                                            meta_info={"request_id": k, "generation_config": gc}))
        st.add_request("STOP", None)
        st.start_server(data=None, request_complete_callback=lambda data: done.__setitem__(data.meta_info["request_id"], data.meta_info))
        return done
    one = dict(base, num_return_sequences=1)
    confs = [dict(one, temperature=0.0), dict(one, temperature=0.0, logprobs=2), dict(one, temperature=1.0, top_k=50, seed=1, logprobs=0),
             dict(base, temperature=1.0, top_k=50, seed=2, num_return_sequences=3, logprobs=1)]
    done = serve(confs)
    assert sorted(done) == [0, 1, 2, 3]
    assert "output_logprobs" not in done[0] and "output_top_logprobs" not in done[0]
    assert "output_top_logprobs" not in done[2]
    for k in (1, 2, 3):
        toks, lps = done[k]["output_token_ids"], done[k]["output_logprobs"]
        assert len(toks) == len(lps) == (3 if k == 3 else 1)
        assert all(len(a) == len(b_) for a, b_ in zip(toks, lps))
    assert all(len(t) == 2 for t in done[1]["output_top_logprobs"][0]) and all(len(t) == 1 for x in done[3]["output_top_logprobs"] for t in x)
    assert done[0]["output_token_ids"] == done[1]["output_token_ids"]          # (one prompt, greedy: asking changes no token)
    assert st.engine.top_logprobs is None          # (the server's batcher handed the engine back with the recording off)
    # requests the rows cannot take (num_return_sequences above max_batch) go through the static list: the records come back with the tokens, for
    # the request that asked and not for the one that did not
    big = dict(base, temperature=1.0, top_k=50, seed=5, num_return_sequences=9)
    done = serve([dict(big, logprobs=2), dict(big)])
    assert sorted(done) == [0, 1]
    assert "output_logprobs" not in done[1] and "output_top_logprobs" not in done[1] and len(done[1]["output_token_ids"]) == 9
    toks, lps, tops = done[0]["output_token_ids"], done[0]["output_logprobs"], done[0]["output_top_logprobs"]
    assert len(toks) == len(lps) == len(tops) == 9
    for a, b_, c in zip(toks, lps, tops):
        assert len(a) == len(b_) == len(c) > 0 and all(len(t) == 2 for t in c) and all(v <= 0 for v in b_)
    assert done[0]["output_token_ids"] == done[1]["output_token_ids"]          # (same prompt, same seed)
    assert st.engine.top_logprobs is None
    st.engine.close()
