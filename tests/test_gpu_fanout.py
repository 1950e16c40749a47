"""GPU tests of n sequences per prompt from ONE admission (the reference's num_return_sequences): the KV prefix fan-out kernel against torch
indexing, the fan-out admission against independent admissions (greedy: bit for bit), its all-ones form against the plain admission, the forks'
first-token draws against the float64 sampler rule, abort of fan-out requests in every state, and the strategy / request-level layers."""
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


def _filtered_probs(logits, temperature, top_k, top_p):
    """the sampler's rule (socioreasoner_amd/sampling.py; tests/test_gpu_parity.py), float64"""
    x = logits.double() / temperature
    kth = torch.topk(x, top_k).values[-1]
    x = torch.where(x < kth, torch.full_like(x, float("-inf")), x)
    sx, si = torch.sort(x, descending=False)
    cp = torch.softmax(sx, -1).cumsum(-1)
    drop = cp <= (1.0 - top_p)
    drop[-1] = False
    sx = sx.masked_fill(drop, float("-inf"))
    return torch.softmax(torch.empty_like(x).scatter_(-1, si, sx), -1)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("d", [1, 7, 127])
def test_kv_fanout_kernel_equals_torch_indexing(d):
    """sr_op_kv_fanout at 36 layers, 2 KV heads, max_ctx 2048: positions [0, L) of the source slot land in every destination slot (given in a
    shuffled order) bit for bit, in both layouts (K rows of 256 B, V^T rows of L x 2 B with a partial last chunk when L % 8 != 0); destination
    positions >= L keep their canary and the source slot is unchanged."""
    from socioreasoner_amd import lib
    Lb = lib.load()
    NL, KVH, CTX = 36, 2, 2048
    S = d + 1
    src = S // 2
    dst = [s for s in range(S) if s != src]
    np.random.default_rng(d).shuffle(dst)
    dst_d = torch.tensor(dst, dtype=torch.int32, device="cuda")
    kc = torch.empty(NL, S, KVH, CTX, 128, dtype=torch.int16, device="cuda")
    vc = torch.empty(NL, S, KVH, 128, CTX, dtype=torch.int16, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(d)
    k_src = torch.randint(-32768, 32767, (NL, KVH, CTX, 128), generator=g, device="cuda", dtype=torch.int16)
    v_src = torch.randint(-32768, 32767, (NL, KVH, 128, CTX), generator=g, device="cuda", dtype=torch.int16)
    canary = 0x5A3C
    try:
        for L in (1, 63, 64, 65, 447, 1700, 2047):
            kc.fill_(canary)
            vc.fill_(canary)
            kc[:, src] = k_src
            vc[:, src] = v_src
            rc = Lb.sr_op_kv_fanout(C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), NL, S * KVH * CTX * 128, KVH, CTX, src,
                                    C.c_void_p(dst_d.data_ptr()), d, L, _sp())
            assert rc == 0, Lb.sr_last_error(None)
            torch.cuda.synchronize()
            assert torch.equal(kc[:, src], k_src) and torch.equal(vc[:, src], v_src), (L, "source slot changed")
            for s in dst:
                assert torch.equal(kc[:, s, :, :L], k_src[:, :, :L]), (L, s, "K prefix")
                assert torch.equal(vc[:, s, :, :, :L], v_src[..., :L]), (L, s, "V prefix")
                assert bool((kc[:, s, :, L:] == canary).all()), (L, s, "K written past L")
                assert bool((vc[:, s, :, :, L:] == canary).all()), (L, s, "V written past L")
        # refused: a fan-out longer than the context, no destination
        dd = C.c_void_p(dst_d.data_ptr())
        assert Lb.sr_op_kv_fanout(C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), NL, S * KVH * CTX * 128, KVH, CTX, src, dd, d, CTX + 1, _sp()) != 0
        assert Lb.sr_op_kv_fanout(C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), NL, S * KVH * CTX * 128, KVH, CTX, src, dd, 0, 5, _sp()) != 0
    finally:
        del kc, vc, k_src, v_src
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the engine's fan-out admission
@pytest.mark.parametrize("size", ["tiny", "3b"])
def test_all_ones_fanout_is_the_plain_admission_and_forks_equal_independent_admissions(size):
    """sr_admit_stage_fanout with every fanout 1 gives the logits, first tokens and decoded tokens of sr_admit_stage; with fanouts (3, 1, 2) the prompt
    logits are the same and every fork decodes (greedy) exactly the tokens of its prompt admitted on its own; bad arguments are refused by name."""
    from socioreasoner_amd import lib
    from socioreasoner_amd.engine import Engine
    geom, vocab = _geom(size)
    MB = 8
    e = Engine(geom, max_patches=64, max_prefill_tokens=512, max_batch=MB, max_ctx=128, max_new_tokens=16, kv_slots=2 * MB)
    e.load_synthetic_weights(seed=0)
    ids, pos = _prompts(np.random.default_rng(71), 3, vocab=vocab)
    max_new = [12, 9, 16]

    def run(slots, rows, fanout, p_ids=ids, p_pos=pos, mn=max_new):
        e.rows_begin()
        lg = e.admit_stage(slots, p_ids, p_pos, mn, fanout=fanout, return_logits=True)
        e.admit_commit(rows)
        for _ in range(4):
            e.rows_step(8)
        fin, cnt = e.rows_poll()
        assert all(fin[r] for r in rows)
        return lg.clone(), [e.row_tokens(r, int(cnt[r])).cpu().tolist() for r in rows]

    lg0, t0 = run([9, 12, 10], [0, 1, 2], None)
    lg1, t1 = run([9, 12, 10], [0, 1, 2], [1, 1, 1])
    assert torch.equal(lg0, lg1) and t0 == t1
    assert [len(t) for t in t0] == max_new
    lg2, t2 = run([8, 15, 3, 9, 11, 4], [5, 0, 7, 1, 2, 3], [3, 1, 2])
    assert torch.equal(lg0, lg2)
    assert t2 == [t0[0]] * 3 + [t0[1]] + [t0[2]] * 2
    # the plain-row form (slot == row) as well
    e.rows_begin()
    e.admit([4, 6, 0, 1, 2, 3], ids, pos, max_new, fanout=[3, 1, 2])
    for _ in range(4):
        e.rows_step(8)
    fin, cnt = e.rows_poll()
    assert [e.row_tokens(r, int(cnt[r])).cpu().tolist() for r in (4, 6, 0, 1, 2, 3)] == [t0[0]] * 3 + [t0[1]] + [t0[2]] * 2
    # refusals, each naming the value
    L_ = lib.load()
    e.rows_begin()
    for fan, slots, msg in (([0, 1, 1], [1, 2], "fanout 0"), ([2, 1, 1], [1, 2, 3, 1], "KV slot 1 given twice"),
                            ([2, 1, 1], [1, 2, 3, 99], "KV slot 99 out of range")):
        with pytest.raises(lib.SocioRError, match=msg):
            e.admit_stage(slots, ids, pos, max_new, fanout=fan)
    with pytest.raises(lib.SocioRError, match="staging capacity"):
        e.admit_stage(list(range(129)), ids[:1], pos[:1], [4], fanout=[129])
    with pytest.raises(lib.SocioRError, match="row 0 given twice"):
        e.admit([0, 0], ids[:1], pos[:1], [4], fanout=[2])
    del L_
    e.close()


def _batch_run(e, reqs, overlap, sampling=None):
    from socioreasoner_amd.serving import ContinuousBatcher
    cb = ContinuousBatcher(e, eos=[], pad_id=0, steps_per_poll=4, overlap=overlap, sampling=sampling)
    out = cb.run(reqs)
    assert cb.idle() and len(cb.free) == e.cfg.max_batch and not cb._parts and not cb.row_fork
    return out, cb


@pytest.mark.parametrize("overlap", [False, True])
def test_greedy_fanout_requests_equal_independent_requests(overlap):
    """ContinuousBatcher, overlapped admission on and off: a mix of n = 1 / 3 / 8 (= max_batch) requests -- 20 sequences through 8 rows, so staged
    forks are committed in portions as rows free up -- gives every fork the tokens its prompt gets as an n = 1 request on the same engine; the
    stats count 5 prompts and 20 sequences; n > max_batch is refused at submit."""
    from socioreasoner_amd.engine import Engine
    from socioreasoner_amd.serving import ContinuousBatcher, Request
    geom, vocab = _geom("tiny")
    MB = 8
    e = Engine(geom, max_patches=64, max_prefill_tokens=512, max_batch=MB, max_ctx=128, max_new_tokens=32, kv_slots=2 * MB)
    e.load_synthetic_weights(seed=0)
    ids, pos = _prompts(np.random.default_rng(72), 5, vocab=vocab)
    ns, mx = [3, 1, 8, 3, 5], [20, 7, 14, 25, 9]
    ref, _ = _batch_run(e, [Request(ids=i, pos3=p, max_new=m) for i, p, m in zip(ids, pos, mx)], overlap)
    got, cb = _batch_run(e, [Request(ids=i, pos3=p, max_new=m, n=n) for i, p, m, n in zip(ids, pos, mx, ns)], overlap)
    for k, n in enumerate(ns):
        want = [ref[k]] * n if n > 1 else ref[k]
        assert got[k] == want, k
    assert cb.stats["admitted_prompts"] == 5 and cb.stats["admitted"] == sum(ns)
    cb2 = ContinuousBatcher(e, eos=[], pad_id=0, overlap=overlap)
    with pytest.raises(ValueError, match="capacity"):
        cb2.submit(Request(ids=ids[0], pos3=pos[0], max_new=4, n=MB + 1))
    e.close()


def test_sampled_fanout_forks():
    """Sampling (temperature 1, top_k 100, top_p 0.8): top_k = 1 is greedy; the same seed gives the same tokens twice; the forks of a prompt are not all
    alike; and the first tokens of 2048 forks of one prompt (16 admissions of 128 forks) follow the float64 rule of the test suite on the admission's
    own logits: every draw inside its support, chi-square over bins of >= 5 expected draws below df + 6 sqrt(2 df), total variation below 0.12."""
    from socioreasoner_amd.engine import Engine
    from socioreasoner_amd.serving import Request
    geom, vocab = _geom("tiny")
    MB = 8
    e = Engine(geom, max_patches=64, max_prefill_tokens=512, max_batch=MB, max_ctx=128, max_new_tokens=32, kv_slots=2 * MB)
    e.load_synthetic_weights(seed=0)
    ids, pos = _prompts(np.random.default_rng(73), 3, vocab=vocab)
    mk = lambda n: [Request(ids=i, pos3=p, max_new=16, n=n) for i, p in zip(ids, pos)]
    greedy, _ = _batch_run(e, mk(1), True)
    k1, _ = _batch_run(e, mk(4), True, {"temperature": 1.0, "top_k": 1, "top_p": 0.8, "seed": 3})
    assert k1 == [[g] * 4 for g in greedy]
    smp = {"temperature": 1.0, "top_k": 100, "top_p": 0.8, "seed": 11}
    a, _ = _batch_run(e, mk(6), True, smp)
    b, _ = _batch_run(e, mk(6), True, smp)
    assert a == b
    for forks in a:
        assert len(forks) == 6 and any(f != forks[0] for f in forks), forks
    e.close()
    # the first-token distribution of 2048 forks
    e = Engine(geom, max_patches=64, max_prefill_tokens=512, max_batch=128, max_ctx=128, max_new_tokens=4)
    e.load_synthetic_weights(seed=0)
    e.rows_begin()
    e.rows_sampling(1.0, 100, 0.8, 5)
    draws, lg = [], None
    for _ in range(16):
        logits = e.admit(list(range(128)), ids[:1], pos[:1], [2], fanout=[128], return_logits=True)
        lg = logits[0].double().cpu() if lg is None else lg
        assert torch.equal(logits[0].double().cpu(), lg)
        e.rows_step(2)
        fin, cnt = e.rows_poll()
        assert fin[:128].all()
        draws += [int(e.row_tokens(r, 1).cpu()[0]) for r in range(128)]
    e.close()
    p = _filtered_probs(lg, 1.0, 100, 0.8)
    N = len(draws)
    freq = torch.bincount(torch.tensor(draws), minlength=lg.numel()).double()
    assert bool((p[freq > 0] > 0).all()), "a draw outside the top-k / top-p support"
    exp = p * N
    big = exp >= 5
    obs_b, exp_b = freq[big], exp[big]
    chi2 = float(((obs_b - exp_b) ** 2 / exp_b).sum())
    rest_o, rest_e = float(freq[~big].sum()), float(exp[~big].sum())
    df = int(big.sum()) - 1
    if rest_e >= 5:
        chi2 += (rest_o - rest_e) ** 2 / rest_e
        df += 1
    assert df >= 1 and chi2 < df + 6 * (2 * df) ** 0.5, (chi2, df)
    tv = 0.5 * float((freq / N - p).abs().sum())
    assert tv < 0.12, tv
    assert len(set(draws)) > 1


def test_abort_fanout_requests_queued_staged_and_running():
    """Overlapped batcher with 4 rows and 8 KV slots: X (n = 4) runs, Z (n = 4) is staged in the spare slots, Y (n = 3) is queued, W (n = 2) waits
    behind it.  Aborting X, Z and Y hits three requests; the batcher goes idle with every row and slot free, reports W alone (its 2 lists, equal to
    W served on its own) and no fork of the others."""
    from socioreasoner_amd.engine import Engine
    from socioreasoner_amd.serving import ContinuousBatcher, Request
    geom, vocab = _geom("tiny")
    e = Engine(geom, max_patches=64, max_prefill_tokens=512, max_batch=4, max_ctx=128, max_new_tokens=64, kv_slots=8)
    e.load_synthetic_weights(seed=0)
    ids, pos = _prompts(np.random.default_rng(74), 4, vocab=vocab)
    reqs = {t: Request(ids=ids[k], pos3=pos[k], max_new=m, n=n, tag=t) for k, (t, n, m) in enumerate((("X", 4, 60), ("Z", 4, 60), ("Y", 3, 60), ("W", 2, 10)))}
    cb = ContinuousBatcher(e, eos=[], pad_id=0, steps_per_poll=4, overlap=True)
    for t in "XZYW":
        cb.submit(reqs[t])
    done = []
    cb.pump(lambda r, toks: done.append((r.tag, toks)))
    assert {r.tag for r in cb.active.values()} == {"X"} and len(cb.active) == 4
    assert cb.staged is not None and {r.tag for r in cb.staged[0]} == {"Z"} and len(cb.staged[0]) == 4
    assert [r.tag for r in cb.pending] == ["Y", "W"]
    assert cb.abort(lambda r: r.tag in ("X", "Z", "Y")) == 3
    pumps = 0
    while not cb.idle():
        cb.pump(lambda r, toks: done.append((r.tag, toks)))
        pumps += 1
        assert pumps < 200
    cb._hand_back()
    assert [t for t, _ in done] == ["W"] and len(done[0][1]) == 2
    assert len(cb.free) == 4 and sorted(cb.free_slots) == list(range(8)) and not cb.row_slot and not cb.row_fork and not cb._parts
    alone, _ = _batch_run(e, [Request(ids=ids[3], pos3=pos[3], max_new=10)], True)
    assert done[0][1] == [alone[0]] * 2
    e.close()


# ------------------------------------------------------------------------------------------------ strategy and request-level serving
def _strategy(max_batch=4):
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


def test_strategy_generate_serves_n_from_one_admission_per_prompt():
    """generate with num_return_sequences 4 (sampled on the device): B x 4 rows, prompt-major, each row carrying its prompt; the batcher admitted B
    prompts as 4 B sequences.  n = 6 above max_batch 4 is split into requests of at most 4.  Greedy n = 4 is four copies of the n = 1 output."""
    from roll.distributed.scheduler.protocol import DataProto
    from socioreasoner_amd.config import geometry_tiny
    geom = geometry_tiny()
    st = _strategy()
    rng = np.random.default_rng(8)
    P, B = 24, 3
    ids = torch.from_numpy(rng.integers(0, 2000, size=(B, P))).long()
    mask = torch.ones(B, P, dtype=torch.long)
    ids[1, :5] = 0
    mask[1, :5] = 0
    batch = DataProto(batch={"input_ids": ids, "attention_mask": mask}, non_tensor_batch={})
    base = dict(max_new_tokens=12, eos_token_id=[2046], pad_token_id=2045, num_beams=1, repetition_penalty=1.0)
    smp = dict(base, temperature=1.0, top_k=100, top_p=0.8, seed=4, num_return_sequences=4)
    a = st.generate(batch, smp)
    assert a.shape[0] == 4 * B and torch.equal(a[:, :P], ids.repeat_interleave(4, dim=0))
    assert st.gen_stats[-1]["admitted_prompts"] == B and st.gen_stats[-1]["admitted"] == 4 * B, st.gen_stats[-1]
    assert torch.equal(a, st.generate(batch, smp))
    assert any(not torch.equal(a[4 * i], a[4 * i + j]) for i in range(B) for j in range(1, 4))
    six = st.generate(batch, dict(smp, num_return_sequences=6))
    assert six.shape[0] == 6 * B and torch.equal(six[:, :P], ids.repeat_interleave(6, dim=0))
    assert st.gen_stats[-1]["admitted"] == 6 * B
    g1 = st.generate(batch, dict(base, temperature=0.0, top_k=-1, top_p=1.0, num_return_sequences=1))
    g4 = st.generate(batch, dict(base, temperature=0.0, top_k=-1, top_p=1.0, num_return_sequences=4))
    assert torch.equal(g4, g1.repeat_interleave(4, dim=0))
    st.engine.close()


def test_request_level_serving_returns_n_lists_per_request(tmp_path):
    """generate_opt_level 1 on the real engine with num_return_sequences 3 (sampled): every request is answered with 3 token lists, and the
    scheduler returns 3 rows per prompt (it used to drop n); greedy at level 1 returns 3 copies of level 0's n = 1 answer."""
    from roll.distributed.scheduler.generate_scheduler import GenerateScheduler
    from roll.distributed.scheduler.protocol import DataProto
    from roll.pipeline.base_worker import ActorWorker
    from tests.test_gpu_pipeline import _cfg
    cfg = _cfg(str(tmp_path), resp=10, prompt=48)
    cfg.actor_infer.generating_args.update({"temperature": 1.0, "top_k": 100, "top_p": 0.8, "max_new_tokens": 10, "num_return_sequences": 3})
    cfg.actor_infer.strategy_args.strategy_config["max_batch"] = 4
    w = ActorWorker(cfg.actor_infer, cfg, 0, 1, 0, "actor_infer").initialize(cfg)
    g = w.strategy.geom
    P, pad, B = 48, g.pad_token_id, 5
    rng = np.random.default_rng(9)
    rows = []
    for i in range(B):
        ids = rng.integers(5, 1500, 10 + 3 * i).astype(np.int64)
        row = np.full(P, pad, dtype=np.int64)
        row[P - len(ids):] = ids
        rows.append(row)
    input_ids = torch.from_numpy(np.stack(rows))
    mask = (input_ids != pad).long()
    pos = (mask.cumsum(-1) - 1).clamp(min=0)[:, None, :].repeat(1, 3, 1)
    fresh = lambda: DataProto(batch={"input_ids": input_ids.clone(), "attention_mask": mask.clone(), "position_ids": pos.clone()}, non_tensor_batch={})
    sched = GenerateScheduler()
    cfg["generate_opt_level"] = 1
    out = sched.generate(fresh(), w, cfg)
    assert out.batch["responses"].shape[0] == 3 * B and torch.equal(out.batch["prompts"], input_ids.repeat_interleave(3, dim=0))
    assert int(out.batch["response_mask"].sum()) > 0
    assert all(len(sched.results[i]) == 3 for i in range(B))
    cfg.actor_infer.generating_args.update({"temperature": 0, "top_k": 1})
    g3 = sched.generate(fresh(), w, cfg)
    cfg["generate_opt_level"] = 0
    cfg.actor_infer.generating_args["num_return_sequences"] = 1
    g1 = sched.generate(fresh(), w, cfg)
    assert torch.equal(g3.batch["responses"], g1.batch["responses"].repeat_interleave(3, dim=0))
    w.strategy.engine.close()
