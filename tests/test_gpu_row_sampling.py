"""GPU tests of per-request sampling in the continuous batcher: the per-row parameter table (k_sample / k_sample_full in one step), the
restated shared key, seed invariance, per-row first-token distributions, the repetition penalty over steps through per-slot bitmaps, the
penalty-aware block shortcut, and the strategy / request-level layers."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _prompts(rng, n, lo=5, hi=40, vocab=2000):
    ids = [rng.integers(0, vocab, int(rng.integers(lo, hi))).astype(np.int64) for _ in range(n)]
    pos = [np.tile(np.arange(len(x)), (3, 1)).astype(np.int64) for x in ids]
    return ids, pos


def _geom(size):
    from socioreasoner_amd.config import geometry_3b, geometry_tiny
    if size == "tiny":
        return geometry_tiny(), 2000
    g = geometry_3b()
    return replace(g, text=replace(g.text, num_hidden_layers=4), vision=replace(g.vision, depth=2, fullatt_block_indexes=(1,))), 150000


def _engine(size="tiny", MB=8, new=32, prefill=512):
    from socioreasoner_amd.engine import Engine
    geom, vocab = _geom(size)
    e = Engine(geom, max_patches=64, max_prefill_tokens=prefill, max_batch=MB, max_ctx=128, max_new_tokens=new, kv_slots=2 * MB)
    e.load_synthetic_weights(seed=0)
    return e, vocab


def _run(e, reqs, overlap, sampling=None, per_row=None):
    from socioreasoner_amd.serving import ContinuousBatcher
    cb = ContinuousBatcher(e, eos=[], pad_id=0, steps_per_poll=4, overlap=overlap, sampling=sampling, per_row=per_row)
    out = cb.run(reqs)
    assert cb.idle() and len(cb.free) == e.cfg.max_batch and not cb.row_own
    return out, cb


def _penalised(lg32, seen, rp):
    """the device's penalty in float32 (l > 0 ? l / rp : l * rp on the seen tokens)"""
    r = torch.tensor(rp, dtype=torch.float32)
    return torch.where(seen, torch.where(lg32 > 0, lg32 / r, lg32 * r), lg32)


def _filtered_probs(x, temperature, top_k, top_p):
    """the sampler's rule (socioreasoner_amd/sampling.py) in float64; top_k <= 0: no top-k bound"""
    x = x.double() / temperature
    if 0 < top_k < x.numel():
        kth = torch.topk(x, top_k).values[-1]
        x = torch.where(x < kth, torch.full_like(x, float("-inf")), x)
    sx, si = torch.sort(x, descending=False)
    cp = torch.softmax(sx, -1).cumsum(-1)
    drop = cp <= (1.0 - top_p)
    drop[-1] = False
    sx = sx.masked_fill(drop, float("-inf"))
    return torch.softmax(torch.empty_like(x).scatter_(-1, si, sx), -1)


def _fits(p, draws):
    """every draw inside the support; chi-square over bins of >= 5 expected draws below df + 6 sqrt(2 df); total variation below twice its
    expectation under the null plus 0.03"""
    N = len(draws)
    freq = torch.bincount(torch.tensor(draws), minlength=p.numel()).double()
    assert bool((p[freq > 0] > 0).all()), "a draw outside the top-k / top-p support"
    exp = p * N
    big = exp >= 5
    chi2 = float(((freq[big] - exp[big]) ** 2 / exp[big]).sum())
    df = int(big.sum()) - 1
    rest_o, rest_e = float(freq[~big].sum()), float(exp[~big].sum())
    if rest_e >= 5:
        chi2 += (rest_o - rest_e) ** 2 / rest_e
        df += 1
    if df >= 1:
        assert chi2 < df + 6 * (2 * df) ** 0.5, (chi2, df)
    tv = 0.5 * float((freq / N - p).abs().sum())
    tv_null = 0.5 * float(torch.sqrt(2 * p * (1 - p) / (np.pi * N)).sum())
    assert tv < 2 * tv_null + 0.03, (tv, tv_null)


# ------------------------------------------------------------------------------------------------ the penalty-aware block shortcut
def _bitmap(seen):
    """bool [B, V] -> int32 words [B, ceil(V / 32)], bit j of word w = token 32 w + j"""
    B, V = seen.shape
    W = (V + 31) // 32
    pad = torch.zeros(B, W * 32, dtype=torch.int64, device=seen.device)
    pad[:, :V] = seen.long()
    w = (pad.view(B, W, 32) << torch.arange(32, device=seen.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


@pytest.mark.parametrize("case", ["filtered", "fallback"])
@pytest.mark.parametrize("rp", [1.05, 1.3, 2.0])
def test_penalised_block_shortcut_equals_the_full_scan(rp, case):
    """sr_op_sample with a seen-token bitmap AND the LM head's block maxima (the shortcut over the blocks whose maximum reaches pen(M_K)) draws
    exactly the tokens of the full-vocabulary scan (no maxima), 16 steps x 8 rows, top_k 100 and 1.  filtered: 300 tall logits in separate
    blocks, half of them seen -- only their blocks reach pen(M_K); fallback: a flat row, every block reaches it (more than KMAX blocks).  The
    draws lie in the penalised top-k, and top_k 1 is the penalised arg-max."""
    from socioreasoner_amd import lib
    L = lib.load()
    B, V, R = 8, 151936, 64
    nb = V // R
    g = torch.Generator(device="cuda").manual_seed(int(rp * 100) + (case == "fallback"))
    seen = torch.rand(B, V, generator=g, device="cuda") < 0.3
    if case == "filtered":
        lg = torch.randn(B, V, generator=g, device="cuda")
        spikes = torch.randperm(nb, generator=g, device="cuda")[:300] * R + 7
        lg[:, spikes] = 20.0 + torch.randn(B, 300, generator=g, device="cuda")
        seen[:, spikes[::2]] = True
    else:
        lg = 5.0 + 0.01 * torch.randn(B, V, generator=g, device="cuda")
    lg = lg.contiguous()
    words = _bitmap(seen)
    bmax = lg.view(B, nb, R).amax(-1).contiguous()
    pen = _penalised(lg, seen, rp)
    out_f = torch.empty(B, dtype=torch.int64, device="cuda")
    out_s = torch.empty(B, dtype=torch.int64, device="cuda")
    for k in (100, 1):
        top = torch.topk(pen, k, dim=-1).indices
        for s in range(16):
            step = torch.full((B,), s, dtype=torch.int32, device="cuda")
            for bm, out in ((bmax, out_s), (None, out_f)):
                rc = L.sr_op_sample(C.c_void_p(lg.data_ptr()), B, V, 1.0, k, 0.9, rp, C.c_void_p(words.data_ptr()), 1234 + s,
                                    C.c_void_p(step.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(bm.data_ptr()) if bm is not None else None,
                                    nb, R, _sp())
                assert rc == 0, L.sr_last_error(None)
            torch.cuda.synchronize()
            assert torch.equal(out_s, out_f), (k, s, out_s.tolist(), out_f.tolist())
            assert bool((top == out_s[:, None]).any(-1).all()), "a draw outside the penalised top-k"
        if k == 1:
            assert torch.equal(out_s, pen.argmax(-1))


# ------------------------------------------------------------------------------------------------ the per-row table in the batcher
@pytest.mark.parametrize("overlap", [False, True])
def test_uniform_table_equals_the_shared_path(overlap):
    """per_row=True with every request on the batcher's configuration: the per-row step replays a uniform table (seed = the batcher's, stream =
    the row, first tokens keyed as sr_admit_stage keys them) and gives the shared sampled step's tokens bit for bit -- fan-out forks included,
    top-k and no-bound nucleus -- and the same for the greedy batcher.  A Request.sampling equal to the batcher's configuration runs on the
    shared step.  Bad entries are refused by name."""
    from socioreasoner_amd import lib
    from socioreasoner_amd.serving import Request
    e, vocab = _engine()
    ids, pos = _prompts(np.random.default_rng(81), 6, vocab=vocab)
    # the shared path keys a row's draws by the row, so the rows a request lands in must not depend on timing: without overlap, 15 sequences
    # churn through 8 rows (admitted as rows free up, at fixed steps); with overlap, when a staged admission lands depends on the device, so
    # all 8 sequences are admitted at once
    ns, mx = ([1, 3, 2, 1, 4, 4], [20, 9, 25, 14, 7, 18]) if not overlap else ([1, 3, 2, 1, 1], [20, 9, 25, 14, 7])
    mk = lambda smp=None: [Request(ids=i, pos3=p, max_new=m, n=n, sampling=smp) for i, p, m, n in zip(ids, pos, mx, ns)]
    for smp in ({"temperature": 0.9, "top_k": 50, "top_p": 0.85, "seed": 21}, {"temperature": 1.0, "top_k": -1, "top_p": 0.9, "seed": 5}):
        ref, cb0 = _run(e, mk(), overlap, smp)
        got, cb = _run(e, mk(), overlap, smp, per_row=True)
        assert got == ref
        assert cb.stats["steps_per_row"] == cb.stats["steps"] > 0 and cb0.stats["steps_per_row"] == 0
        same, cb2 = _run(e, mk({k: v for k, v in smp.items() if k != "seed"}), overlap, smp)
        assert same == ref and cb2.stats["steps_per_row"] == 0
        assert any(f != forks[0] for forks in ref if isinstance(forks[0], list) for f in forks)
    g_ref, _ = _run(e, mk(), overlap)
    g_got, _ = _run(e, mk(), overlap, per_row=True)
    assert g_got == g_ref
    e.rows_begin()
    for bad, msg in (((-1.0, 10, 0.9, 1.0, 0, 0), "temperature"), ((1.0, 1025, 0.9, 1.0, 0, 0), "top_k 1025"),
                     ((1.0, 10, 0.0, 1.0, 0, 0), "top_p"), ((1.0, 10, 1.5, 1.0, 0, 0), "top_p"), ((1.0, 10, 0.9, 0.0, 0, 0), "repetition_penalty")):
        with pytest.raises(lib.SocioRError, match=msg):
            e.admit([0], ids[:1], pos[:1], [4], sampling=[bad])
    e.close()


@pytest.mark.parametrize("size", ["tiny", "3b"])
def test_greedy_rows_in_a_mixed_batch_equal_the_all_greedy_batcher(size):
    """Greedy requests decoded beside top-k, no-bound nucleus, penalised and penalised-greedy rows (overlap on; 8 rows tiny, 32 rows of the
    4-layer 3B geometry) get exactly their tokens from a batcher that serves only them."""
    from socioreasoner_amd.serving import Request
    MB = 8 if size == "tiny" else 32
    e, vocab = _engine(size, MB=MB, new=24, prefill=512 if size == "tiny" else 2048)
    rng = np.random.default_rng(82)
    n_req = 3 * MB // 2
    ids, pos = _prompts(rng, n_req, vocab=vocab)
    mx = [int(rng.integers(4, 24)) for _ in range(n_req)]
    confs = [None, {"temperature": 1.0, "top_k": 100, "top_p": 0.8}, {"temperature": 0.7, "top_k": -1, "top_p": 0.95, "repetition_penalty": 1.2},
             {"temperature": 0.0, "repetition_penalty": 1.3}]
    gi = [k for k in range(n_req) if k % 4 == 0]
    ref, _ = _run(e, [Request(ids=ids[k], pos3=pos[k], max_new=mx[k]) for k in gi], True)
    got, cb = _run(e, [Request(ids=ids[k], pos3=pos[k], max_new=mx[k], sampling=confs[k % 4], n=2 if k % 4 == 1 else 1) for k in range(n_req)], True)
    assert [got[k] for k in gi] == ref
    assert cb.stats["steps_per_row"] > 0
    pg = [got[k] for k in range(n_req) if k % 4 == 3]
    assert pg != [got[k] for k in gi]
    e.close()


def test_seeded_request_does_not_depend_on_row_slot_or_neighbours():
    """A request with its own seed (n = 3, top-k 64, top-p 0.9, penalty 1.1) gives the same three token lists served alone, inside a churning
    mixed batch where it waits for rows and is admitted at another step into other rows and slots (overlap on), and after other neighbours
    without overlap; its forks differ from each other."""
    from socioreasoner_amd.serving import Request
    e, vocab = _engine(new=32)
    rng = np.random.default_rng(83)
    ids, pos = _prompts(rng, 14, vocab=vocab)
    own = {"temperature": 1.0, "top_k": 64, "top_p": 0.9, "repetition_penalty": 1.1, "seed": 777}
    X = lambda: Request(ids=ids[0], pos3=pos[0], max_new=24, n=3, sampling=dict(own))
    alone, _ = _run(e, [X()], True)
    confs = [None, {"temperature": 0.8, "top_k": 20, "top_p": 1.0}, {"temperature": 0.0, "repetition_penalty": 1.3}, {"temperature": 1.2, "top_k": 0, "top_p": 0.9}]
    others = [Request(ids=ids[k], pos3=pos[k], max_new=int(rng.integers(3, 30)), sampling=confs[k % 4], n=1 + k % 2) for k in range(1, 14)]
    got, _ = _run(e, others[:7] + [X()] + others[7:], True, {"temperature": 1.0, "top_k": 100, "top_p": 0.8, "seed": 3})
    assert got[7] == alone[0]
    got2, _ = _run(e, others[:3] + [X()], False)
    assert got2[3] == alone[0]
    assert len({tuple(f) for f in alone[0]}) > 1
    e.close()


def test_per_row_first_tokens_follow_their_own_distributions():
    """One prompt fanned out into 128 forks per admission under four (T, top_k, top_p, rp) settings, 32 forks each, 24 admissions: each
    group's first tokens follow its own float64 filtered distribution of the admission logits with the prompt tokens penalised."""
    from socioreasoner_amd.engine import Engine
    geom, vocab = _geom("tiny")
    e = Engine(geom, max_patches=64, max_prefill_tokens=512, max_batch=128, max_ctx=128, max_new_tokens=4)
    e.load_synthetic_weights(seed=0)
    ids, pos = _prompts(np.random.default_rng(84), 1, vocab=vocab)
    groups = [(1.0, 100, 0.8, 1.0), (0.7, 20, 1.0, 1.3), (1.5, -1, 0.9, 1.0), (1.0, 0, 0.95, 2.0)]
    e.rows_begin()
    e.rows_per_row(True)
    draws, lg = [[] for _ in groups], None
    for a in range(24):
        ent = [groups[j % 4] + (1000 + a, j) for j in range(128)]
        logits = e.admit(list(range(128)), ids, pos, [2], fanout=[128], return_logits=True, sampling=ent)
        lg = logits[0].cpu() if lg is None else lg
        assert torch.equal(logits[0].cpu(), lg)
        e.rows_step(2)
        fin, cnt = e.rows_poll()
        assert fin[:128].all()
        first = e.rows_tokens(list(range(128)), [1] * 128)[:, 0].cpu().tolist()
        for j, t in enumerate(first):
            draws[j % 4].append(int(t))
    e.close()
    seen = torch.zeros(lg.numel(), dtype=torch.bool)
    seen[torch.from_numpy(ids[0])] = True
    for (t, k, p, rp), d in zip(groups, draws):
        _fits(_filtered_probs(_penalised(lg, seen, rp), t, k, p), d)
        assert len(set(d)) > 1


def test_repetition_penalty_rows_equal_the_static_path():
    """Greedy with repetition_penalty 1.3 in rows mode (n = 2 fan-out, after aborting requests that held rows and KV slots, so their slots are
    reused) equals the static path (sr_decode_sample with top_k 1 on a 32-row static batch, the same decode kernels) token for token; the
    plain greedy decode repeats tokens and the penalised one differs from it."""
    from socioreasoner_amd.serving import ContinuousBatcher, Request
    e, vocab = _engine(MB=32, new=24, prefill=2048)
    rng = np.random.default_rng(85)
    ids, pos = _prompts(rng, 16, vocab=vocab)
    N = 24
    sid, spos = [x for x in ids for _ in range(2)], [p for p in pos for _ in range(2)]
    e.prefill(sid, spos)
    plain = e.decode(N).cpu().tolist()
    e.prefill(sid, spos)
    pen = e.decode_sample(N, 1.0, 1, 1.0, repetition_penalty=1.3, seed=0).cpu().tolist()
    assert any(len(set(r)) < len(r) for r in plain), "the plain greedy decode does not repeat: the test would be vacuous"
    assert pen != plain and sum(len(set(r)) for r in pen) > sum(len(set(r)) for r in plain)
    own = {"temperature": 0.0, "repetition_penalty": 1.3}
    cb = ContinuousBatcher(e, eos=[], pad_id=0, steps_per_poll=4, overlap=True)
    jid, jpos = _prompts(rng, 4, vocab=vocab)
    for i, p in zip(jid, jpos):
        cb.submit(Request(ids=i, pos3=p, max_new=N, n=8, sampling=dict(own), tag="junk"))
    out = {}
    cb.pump(lambda r, t: None)
    cb.pump(lambda r, t: None)
    assert cb.abort(lambda r: r.tag == "junk") >= 1
    for k in range(16):
        cb.submit(Request(ids=ids[k], pos3=pos[k], max_new=N, n=2, sampling=dict(own), tag=k))
    while not cb.idle():
        cb.pump(lambda r, t: out.__setitem__(r.tag, t) if r.tag != "junk" else None)
    cb._hand_back()
    for k in range(16):
        assert out[k] == [pen[2 * k], pen[2 * k + 1]], k
    e.close()


# ------------------------------------------------------------------------------------------------ strategy and request-level serving
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


def test_strategy_generate_with_a_repetition_penalty_uses_the_batcher():
    """generate with repetition_penalty 1.05 and n = 4 (sampled): B x 4 rows from B admissions of the continuous batcher (no static prefill),
    reproducible; greedy with penalty 1.3 and n = 2: also through the batcher, n copies of one answer per prompt."""
    from roll.distributed.scheduler.protocol import DataProto
    st = _strategy()
    rng = np.random.default_rng(8)
    P, B = 24, 3
    ids = torch.from_numpy(rng.integers(0, 2000, size=(B, P))).long()
    batch = DataProto(batch={"input_ids": ids, "attention_mask": torch.ones(B, P, dtype=torch.long)}, non_tensor_batch={})
    calls, orig = [], st.engine.prefill
    st.engine.prefill = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    base = dict(max_new_tokens=12, eos_token_id=[2046], pad_token_id=2045, num_beams=1)
    smp = dict(base, temperature=1.0, top_k=100, top_p=0.8, seed=4, num_return_sequences=4, repetition_penalty=1.05)
    a = st.generate(batch, smp)
    assert a.shape[0] == 4 * B and torch.equal(a[:, :P], ids.repeat_interleave(4, dim=0))
    assert st.gen_stats[-1]["admitted_prompts"] == B and st.gen_stats[-1]["admitted"] == 4 * B, st.gen_stats[-1]
    assert torch.equal(a, st.generate(batch, smp))
    g = st.generate(batch, dict(base, temperature=0.0, top_k=-1, top_p=1.0, num_return_sequences=2, repetition_penalty=1.3))
    assert g.shape[0] == 2 * B and torch.equal(g[0::2], g[1::2]) and st.gen_stats[-1]["admitted_prompts"] == B
    assert not calls
    st.engine.close()


def test_start_server_serves_mixed_configs_in_one_batcher():
    """start_server fed interleaved greedy, sampled (top-k), sampled-with-penalty and greedy-with-penalty requests serves them all without
    calling the static generate; the greedy answers equal a greedy-only run; two seedless penalised requests with the same prompt differ."""
    from roll.distributed.scheduler.protocol import DataProto
    st = _strategy()
    calls, orig = [], st.generate
    st.generate = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    rng = np.random.default_rng(86)
    P, n_req = 24, 16
    prompts = [torch.from_numpy(rng.integers(0, 2000, size=(1, P))).long() for _ in range(n_req)]
    prompts[14] = prompts[10].clone()          # two seedless sampled, penalised requests with one prompt
    base = dict(max_new_tokens=12, eos_token_id=[2046], pad_token_id=2045, num_beams=1, num_return_sequences=1)
    confs = [dict(base, temperature=0.0, top_k=-1, top_p=1.0), dict(base, temperature=1.0, top_k=100, top_p=0.8, seed=3),
             dict(base, temperature=0.8, top_k=-1, top_p=0.9, repetition_penalty=1.2), dict(base, temperature=0.0, repetition_penalty=1.3)]

    def serve(ks):
        done = {}
        for k in ks:
            st.add_request("ADD", DataProto(batch={"input_ids": prompts[k], "attention_mask": torch.ones_like(prompts[k])}, non_tensor_batch={},
                                            meta_info={"request_id": k, "generation_config": confs[k % 4]}))
        st.add_request("STOP", None)
        st.start_server(data=None, request_complete_callback=lambda data: done.__setitem__(data.meta_info["request_id"], data.meta_info["output_token_ids"]))
        return done

    mixed = serve(range(n_req))
    assert sorted(mixed) == list(range(n_req)) and not calls
    greedy = serve([k for k in range(n_req) if k % 4 == 0])
    assert all(mixed[k] == greedy[k] for k in greedy)
    assert mixed[10] != mixed[14]
    st.engine.close()
