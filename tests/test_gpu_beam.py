"""GPU tests of beam search on the device (sr_decode_beam; the reference's num_beams > 1 with HF's semantics): the select kernel against the host
restatement fed with the device's own logits, the KV reorder checked independently by teacher forcing every hypothesis, the suffix-copy
kernel against torch indexing, batch invariance, graph replay against eager launches, and the strategy / request-level layers."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from tests.beam_ref import beam_search_ref

pytestmark = pytest.mark.gpu


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


def _engine(size, MB, max_new, max_ctx=256):
    from socioreasoner_amd.engine import Engine
    geom, vocab = _geom(size)
    e = Engine(geom, max_patches=64, max_prefill_tokens=1024, max_batch=MB, max_ctx=max_ctx, max_new_tokens=max_new)
    e.load_synthetic_weights(seed=0)
    return e, vocab


def _eos_for(e, ids, pos, W, n_eos):
    """eos tokens that the beams actually meet: the most likely first tokens of the first prompt after its top candidate"""
    lg = e.prefill(ids[:1], pos[:1], return_logits=True)[0]
    order = torch.argsort(lg, descending=True).tolist()
    return [int(t) for t in order[1:1 + n_eos]]


CASES = [("tiny", 2, 1, 3, 1.0), ("tiny", 4, 2, 2, 0.0), ("tiny", 8, 1, 4, 2.0), ("3b", 4, 1, 2, 1.0), ("3b", 8, 2, 1, 1.0)]


@pytest.mark.parametrize("size,W,n_eos,G,lp", CASES)
def test_beam_select_matches_restatement_on_device_logits(size, W, n_eos, G, lp):
    """sr_decode_beam with its logits trace: the host restatement fed those logits reproduces the device's parents, tokens (trace), stop steps,
    returned sequences and lengths exactly and its scores within 1e-5; graph replay gives the eager result bit for bit."""
    max_new = 24
    e, vocab = _engine(size, 32, max_new)
    ids, pos = _prompts(np.random.default_rng(100 + W + G), G, vocab=vocab)
    eos = _eos_for(e, ids, pos, W, n_eos)
    R = min(2, W)
    e.prefill(ids, pos)
    toks, scores, lens = e.decode_beam(W, max_new, R, lp, eos=eos, pad_id=vocab - 1, trace=True)
    steps = e.steps_done
    lg = e.beam_logits.cpu()
    tr = e.beam_trace.cpu()
    ref = beam_search_ref(lambda t: lg[t], G, W, R, max_new, eos, vocab - 1, lp)
    assert ref["steps"] == steps
    dev_tr = [[tuple(x) for x in tr[t].tolist()] for t in range(steps)]
    assert dev_tr == ref["trace"]
    assert (tr[steps:] == -1).all()
    for g in range(G):
        for r in range(R):
            n = int(lens[g, r])
            assert n == ref["lengths"][g][r]
            assert toks[g, r, :n].tolist() == ref["tokens"][g][r]
            assert (toks[g, r, n:] == vocab - 1).all()
            assert abs(float(scores[g, r]) - ref["scores"][g][r]) <= 1e-5 * max(1.0, abs(ref["scores"][g][r]))   # (float32: lp = 0 sums reach ~100)
    e.prefill(ids, pos)
    toks2, scores2, lens2 = e.decode_beam(W, max_new, R, lp, eos=eos, pad_id=vocab - 1, use_graph=True)
    assert torch.equal(toks, toks2) and torch.equal(scores, scores2) and torch.equal(lens, lens2)
    e.close()


def test_beam_32_rows_eos_ends_beams_and_real_copies_happen():
    """4 groups x 8 beams = 32 rows, one eos that the beams meet, length_penalty 0 (short hypotheses compete): eos ends hypotheses early, the
    restatement agrees, and the run contains steps where a parent had two or more children while another had none (so the KV suffix copies ran)."""
    e, vocab = _engine("tiny", 32, 32)
    G, W, R, max_new = 4, 8, 3, 32
    ids, pos = _prompts(np.random.default_rng(5), G, lo=9, hi=30, vocab=vocab)
    eos = _eos_for(e, ids, pos, W, 1)
    e.prefill(ids, pos)
    toks, scores, lens = e.decode_beam(W, max_new, R, 0.0, eos=eos, pad_id=vocab - 1, trace=True)
    lg, tr = e.beam_logits.cpu(), e.beam_trace.cpu()
    ref = beam_search_ref(lambda t: lg[t], G, W, R, max_new, eos, vocab - 1, 0.0)
    assert [[tuple(x) for x in tr[t].tolist()] for t in range(e.steps_done)] == ref["trace"]
    assert any(f[1] + 1 < max_new for g in range(G) for f in ref["fin"][g]), "no hypothesis ended on eos"
    assert any(int(lens[g, r]) < max_new for g in range(G) for r in range(R))
    assert _reorder_steps(tr[:e.steps_done], G, W) > 0
    e.close()


def _reorder_steps(tr, G, W):
    n = 0
    for t in range(1, tr.shape[0]):
        for g in range(G):
            par = tr[t, g * W:(g + 1) * W, 0].tolist()
            if par[0] < 0:
                continue
            cnt = [par.count(p) for p in range(W)]
            n += max(cnt) >= 2 and min(cnt) == 0
    return n


@pytest.mark.parametrize("size,W,lp", [("tiny", 4, 1.0), ("3b", 4, 2.0), ("tiny", 8, 0.0)])
def test_kv_reorder_teacher_forced_scores(size, W, lp):
    """Every returned hypothesis, teacher-forced through plain sr_decode from a fresh prefill at the beam run's row count: its summed log-probs
    over len ** lp equal the beam score within 1e-4.  Prompt lengths with L % 8 != 0 hit the partial V^T chunk; real copies happened."""
    max_new = 20
    G = 32 // W
    e, vocab = _engine(size, 32, max_new)
    ids, pos = _prompts(np.random.default_rng(11 + W), G, lo=9, hi=45, vocab=vocab)
    assert any(len(x) % 8 for x in ids)
    pad = vocab - 1
    e.prefill(ids, pos)
    toks, scores, lens = e.decode_beam(W, max_new, W, lp, eos=[], pad_id=pad, trace=True)
    assert _reorder_steps(e.beam_trace.cpu()[:e.steps_done], G, W) > 0
    hyps = [(g, r) for g in range(G) for r in range(W)]
    assert len(hyps) == G * W
    f_ids = [ids[g] for g, _ in hyps]
    f_pos = [pos[g] for g, _ in hyps]
    forced = torch.stack([toks[g, r] for g, r in hyps]).to(torch.int32)
    e.prefill(f_ids, f_pos)
    _, lg = e.decode(max_new, eos=[], pad_id=pad, trace=True, forced=forced, use_graph=False)
    lp_all = torch.log_softmax(lg.cpu().double(), dim=-1)
    for b, (g, r) in enumerate(hyps):
        n = int(lens[g, r])
        s = sum(float(lp_all[t, b, int(forced[b, t])]) for t in range(n))
        assert abs(s / n ** lp - float(scores[g, r])) <= 1e-4 * max(1.0, abs(s / n ** lp)), (g, r, s, float(scores[g, r]))
    e.close()


def test_kv_suffix_copy_kernel_equals_torch_indexing():
    """sr_op_kv_suffix_copy at 36 layers, 2 KV heads, max_ctx 2048: [L0, L1) of every entry's source lands in its destination in both layouts
    (unaligned ends: partial V^T chunks); other positions, the sources and untouched slots keep their canaries."""
    from socioreasoner_amd import lib
    Lb = lib.load()
    NL, KVH, CTX, S = 36, 2, 2048, 6
    g = torch.Generator(device="cuda").manual_seed(3)
    kc = torch.randint(-30000, 30000, (NL, S, KVH, CTX, 128), dtype=torch.int16, device="cuda", generator=g)
    vc = torch.randint(-30000, 30000, (NL, S, KVH, 128, CTX), dtype=torch.int16, device="cuda", generator=g)
    k0, v0 = kc.clone(), vc.clone()
    copies = [(0, 3, 13, 77), (1, 4, 40, 41), (2, 5, 1000, 1203), (-1, 2, 0, 9)]
    cd = torch.tensor(copies, dtype=torch.int32, device="cuda")
    lib.check(Lb.sr_op_kv_suffix_copy(kc.data_ptr(), vc.data_ptr(), NL, S * KVH * CTX * 128, KVH, CTX, cd.data_ptr(), len(copies), 203,
                                      torch.cuda.current_stream().cuda_stream), None, "sr_op_kv_suffix_copy")
    torch.cuda.synchronize()
    for s_, d, a, b in copies:
        if s_ < 0:
            continue
        k0[:, d, :, a:b] = k0[:, s_, :, a:b]
        v0[:, d, :, :, a:b] = v0[:, s_, :, :, a:b]
    assert torch.equal(kc, k0) and torch.equal(vc, v0)


def test_beam_batch_invariance():
    """Prompt p's hypotheses, scores and lengths are bit-identical between the batches [p, q1, q2, q3] and [p, r1, r2, r3]."""
    e, vocab = _engine("3b", 16, 16)
    ids, pos = _prompts(np.random.default_rng(21), 7, vocab=vocab)
    out = []
    for sel in ([0, 1, 2, 3], [0, 4, 5, 6]):
        e.prefill([ids[k] for k in sel], [pos[k] for k in sel])
        t, s, l = e.decode_beam(4, 16, 4, 1.0, eos=[], pad_id=0)
        out.append((t[0], s[0], l[0]))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    e.close()


def test_beam_refusals_name_the_value():
    e, vocab = _engine("tiny", 8, 8)
    ids, pos = _prompts(np.random.default_rng(2), 3, vocab=vocab)
    for kw, word in ((dict(num_beams=4), "max_batch"), (dict(num_beams=9), "W=9"), (dict(num_beams=2, num_return_sequences=3), "R=3")):
        e.prefill(ids, pos)
        with pytest.raises(Exception, match=word):
            e.decode_beam(kw["num_beams"], 8, kw.get("num_return_sequences", 1), eos=[])
    e.prefill(ids[:1], pos[:1])
    with pytest.raises(Exception, match="K ="):
        e.decode_beam(8, 8, 1, eos=list(range(8)))
    e.close()


def _strategy(max_batch=8):
    from roll.distributed.strategy.factory import create_strategy

    class W:
        rank, world_size = 0, 1
        pipeline_config = type("P", (), {"prompt_length": 64, "response_length": 16})()
        worker_config = type("C", (), {"strategy_args": type("S", (), {"strategy_name": "mi355x", "strategy_config": {"max_batch": max_batch, "max_ctx": 128}})(),
                                       "model_args": type("M", (), {"model_name_or_path": "synthetic:tiny"})()})()
        rank_info = type("R", (), {"local_rank": 0})()
    st = create_strategy(W())
    st.initialize(None)
    return st


def test_strategy_generate_beam_layout_equals_decode_beam():
    """generate with num_beams=4, num_return_sequences=2: [B*2, P + L], a prompt's 2 sequences adjacent and best first, cut after eos and
    right-padded, equal to decode_beam on the same prompts (chunks of max_batch // 4 prompts)."""
    from roll.distributed.scheduler.protocol import DataProto
    st = _strategy(8)
    rng = np.random.default_rng(8)
    P, B = 24, 3
    ids = torch.from_numpy(rng.integers(0, 2000, size=(B, P))).long()
    mask = torch.ones(B, P, dtype=torch.long)
    ids[1, :5] = 0
    mask[1, :5] = 0
    batch = DataProto(batch={"input_ids": ids, "attention_mask": mask}, non_tensor_batch={})
    eos, pad = [2046], 2045
    gc = dict(max_new_tokens=12, eos_token_id=eos, pad_token_id=pad, num_beams=4, num_return_sequences=2, length_penalty=1.0)
    out = st.generate(batch, gc)
    assert out.shape[0] == 2 * B and torch.equal(out[:, :P], ids.repeat_interleave(2, dim=0))
    prompts = [ids[b][mask[b].bool()].numpy() for b in range(B)]
    exp = []
    for c0 in range(0, B, 2):
        chunk = prompts[c0:c0 + 2]
        st.engine.prefill(chunk, [np.tile(np.arange(len(x)), (3, 1)) for x in chunk])
        t, _, l = st.engine.decode_beam(4, 12, 2, 1.0, eos=eos, pad_id=pad)
        exp += [t[g, r, :int(l[g, r])].tolist() for g in range(len(chunk)) for r in range(2)]
    for row, x in zip(out, exp):
        resp = row[P:].tolist()
        assert resp[:len(x)] == x and all(v == pad for v in resp[len(x):])
    for kw, word in ((dict(repetition_penalty=1.2), "repetition_penalty"), (dict(num_return_sequences=5), "num_return_sequences"),
                     (dict(early_stopping=True), "early_stopping")):
        with pytest.raises((ValueError, NotImplementedError), match=word):
            st.generate(batch, dict(gc, **kw))
    st.engine.close()


def test_request_level_serving_beam(tmp_path):
    """start_server (generate_opt_level 1) with num_beams=4, num_return_sequences=2: every request is answered with 2 token lists, equal to
    level 0's generate; a greedy num_beams=4 request returns the beam result, not the greedy one."""
    from roll.distributed.scheduler.generate_scheduler import GenerateScheduler
    from roll.distributed.scheduler.protocol import DataProto
    from roll.pipeline.base_worker import ActorWorker
    from tests.test_gpu_pipeline import _cfg
    cfg = _cfg(str(tmp_path), resp=10, prompt=48)
    cfg.actor_infer.generating_args.update({"temperature": 0, "top_k": 1, "max_new_tokens": 10, "num_return_sequences": 2, "num_beams": 4})
    cfg.actor_infer.strategy_args.strategy_config["max_batch"] = 8
    w = ActorWorker(cfg.actor_infer, cfg, 0, 1, 0, "actor_infer").initialize(cfg)
    g = w.strategy.geom
    P, pad, B = 48, g.pad_token_id, 3
    rng = np.random.default_rng(9)
    rows = []
    for i in range(B):
        x = rng.integers(5, 1500, 10 + 3 * i).astype(np.int64)
        row = np.full(P, pad, dtype=np.int64)
        row[P - len(x):] = x
        rows.append(row)
    input_ids = torch.from_numpy(np.stack(rows))
    mask = (input_ids != pad).long()
    pos = (mask.cumsum(-1) - 1).clamp(min=0)[:, None, :].repeat(1, 3, 1)
    fresh = lambda: DataProto(batch={"input_ids": input_ids.clone(), "attention_mask": mask.clone(), "position_ids": pos.clone()}, non_tensor_batch={})
    sched = GenerateScheduler()
    cfg["generate_opt_level"] = 1
    b1 = sched.generate(fresh(), w, cfg)
    assert all(len(sched.results[i]) == 2 for i in range(B))
    cfg["generate_opt_level"] = 0
    b0 = sched.generate(fresh(), w, cfg)
    assert torch.equal(b1.batch["responses"], b0.batch["responses"])
    cfg.actor_infer.generating_args.update({"num_return_sequences": 1, "num_beams": 1})
    gr = sched.generate(fresh(), w, cfg)
    assert not torch.equal(gr.batch["responses"], b0.batch["responses"][::2])
    w.strategy.engine.close()
