"""CPU tests of per-request sampling on the host: which requests of the real request loop (start_server) go to the continuous batcher and which
to the static path, what the batcher hands the engine (per-sequence entries, seeds and streams, the per-row switch), and the refusals at submit.
The engine is scripted: row r emits 1000 * (fork + 1) + k at its k-th step."""
import queue
from types import SimpleNamespace

import numpy as np
import pytest
import torch


class ScriptedEngine:
    """the batcher's engine surface (non-overlapped path), recording what it is asked"""

    def __init__(self, max_batch=4):
        self.cfg = SimpleNamespace(max_batch=max_batch, max_prefill_tokens=4096, max_patches=0, max_ctx=256, max_new_tokens=64)
        self.kv_slots, self.device = max_batch, "cpu"
        self.log, self.per_row, self.rows = [], False, {}

    def rows_begin(self):
        self.rows, self.per_row = {}, False
        self.log.append(("begin",))

    def rows_sampling(self, t, k, p, seed):
        self.log.append(("sampling", t, k, p, seed))

    def rows_per_row(self, on):
        self.per_row = bool(on)
        self.log.append(("per_row", self.per_row))

    def admit(self, rows, ids, pos3, max_new, emb=None, fanout=None, sampling=None):
        self.log.append(("admit", [int(x[-1]) for x in ids], None if sampling is None else list(sampling)))
        k = 0
        for i, m in enumerate(max_new):
            for j in range((fanout or [1] * len(ids))[i]):
                self.rows[rows[k]] = [j, int(m), 0]
                k += 1

    def rows_step(self, n, eos, pad):
        self.log.append(("step", n, self.per_row))
        for st in self.rows.values():
            st[2] = min(st[2] + n, st[1])

    def rows_poll(self):
        fin = np.ones(self.cfg.max_batch, dtype=np.int32)
        cnt = np.zeros(self.cfg.max_batch, dtype=np.int32)
        for r, (j, m, c) in self.rows.items():
            fin[r], cnt[r] = int(c >= m), c
        return fin, cnt

    def row_tokens(self, row, n):
        j = self.rows.pop(row)[0]
        return torch.tensor([1000 * (j + 1) + k for k in range(n)], dtype=torch.int32)


def _req(first, n=1, max_new=6, sampling=None):
    from socioreasoner_amd.serving import Request
    ids = np.array([5, 6, 7, first], dtype=np.int64)
    return Request(ids=ids, pos3=np.tile(np.arange(4), (3, 1)), max_new=max_new, n=n, sampling=sampling)


def test_batcher_entries_streams_and_per_row_switch():
    """Requests without parameters run on the shared step; one with its own parameters makes the admission carry per-sequence entries (the
    shared ones keyed by the row, stream -1; its own on streams (seed, fork)) and switches the per-row step on while it runs and off after.  A
    dict equal to the batcher's configuration is the batcher's.  Seedless requests get distinct seeds."""
    from socioreasoner_amd.serving import ContinuousBatcher
    e = ScriptedEngine(max_batch=4)
    smp = {"temperature": 1.0, "top_k": 50, "top_p": 0.9, "seed": 9}
    cb = ContinuousBatcher(e, eos=[], pad_id=0, steps_per_poll=2, sampling=smp)
    reqs = [_req(10), _req(11, sampling={"temperature": 1.0, "top_k": 50, "top_p": 0.9}),
            _req(12, n=2, sampling={"temperature": 0.5, "top_k": -1, "top_p": 0.8, "repetition_penalty": 1.2, "seed": 77})]
    out = cb.run(reqs)
    assert out[0] == [1000 + k for k in range(6)] and out[2] == [[1000 + k for k in range(6)], [2000 + k for k in range(6)]]
    adm = [x for x in e.log if x[0] == "admit"]
    assert len(adm) == 1 and adm[0][1] == [10, 11, 12]
    assert adm[0][2] == [(1.0, 50, 0.9, 1.0, 9, -1), (1.0, 50, 0.9, 1.0, 9, -1), (0.5, -1, 0.8, 1.2, 77, 0), (0.5, -1, 0.8, 1.2, 77, 1)]
    steps = [x for x in e.log if x[0] == "step"]
    assert steps and all(s[2] for s in steps) and cb.stats["steps_per_row"] == cb.stats["steps"]
    # only the batcher's requests: the shared step, plain admissions
    e.log.clear()
    cb.run([_req(13), _req(14, sampling={"temperature": 1.0, "top_k": 50, "top_p": 0.9})])
    assert not any(x[0] == "step" and x[2] for x in e.log) and all(x[2] is None for x in e.log if x[0] == "admit")
    # seedless requests with their own parameters: distinct seeds, streams = fork index; greedy with a penalty: temperature 0
    own = {"temperature": 0.7, "top_k": 20, "repetition_penalty": 1.1}
    a, b = cb._entries(_req(1, n=2, sampling=dict(own))), cb._entries(_req(1, n=2, sampling=dict(own)))
    assert a[0][4] != b[0][4] and [x[5] for x in a] == [0, 1] and a[0][:4] == (0.7, 20, 1.0, 1.1)
    assert cb._entries(_req(1, sampling={"temperature": 0.0, "repetition_penalty": 1.3}))[0][:4] == (0.0, 1, 1.0, 1.3)


def test_submit_refuses_values_outside_the_engine_limits():
    from socioreasoner_amd.serving import ContinuousBatcher
    cb = ContinuousBatcher(ScriptedEngine(), eos=[], pad_id=0)
    for s, word in (({"temperature": -1.0}, "temperature"), ({"temperature": 1.0, "top_k": 2000}, "top_k"), ({"temperature": 1.0, "top_p": 1.5}, "top_p"),
                    ({"temperature": 1.0, "repetition_penalty": 0.0}, "repetition_penalty")):
        with pytest.raises(ValueError, match=word):
            cb.submit(_req(1, sampling=s))
    assert not cb.pending


def test_request_loop_routes_differing_configs_into_the_running_batcher(tmp_path):
    """The real start_server over the scripted engine: greedy, sampled and penalised requests (with and without their own seed) all join ONE
    batcher; a different eos set, num_beams > 1 and top_k above 1024 keep the static path (the scripted generate), which is called with exactly
    those requests."""
    from roll.distributed.scheduler.protocol import DataProto
    from roll.distributed.strategy.mi355x_strategy import Mi355xStrategy
    from roll.pipeline.base_worker import ActorWorker
    from socioreasoner_amd import hostops
    from socioreasoner_amd.config import geometry_tiny
    from socioreasoner_amd.textproc import ByteTokenizer
    from tests.test_host_cpu import _tiny_cfg
    cfg = _tiny_cfg(tmp_path, prompt_length=12, response_length=6)
    tok = ByteTokenizer(geometry_tiny())
    eng = ScriptedEngine(max_batch=4)
    static = []

    class Fake(Mi355xStrategy):
        max_batch = 4

        def initialize(self, model_provider=None):
            self.command_queue, self.tokenizer, self.geom = queue.Queue(), tok, geometry_tiny()
            self.engine, self.overlap = eng, False

        def generate(self, batch, generation_config):
            ids = batch.batch["input_ids"]
            static.extend(int(r[-1]) for r in ids)
            k = int(generation_config.get("num_return_sequences", 1) or 1)
            rows = [[7, tok.eos_token_id] for _ in range(len(ids)) for _ in range(k)]
            out = hostops.gather_outputs_to_pad_tensor(rows, generation_config["pad_token_id"], device=ids.device)
            return hostops.concatenate_input_and_output(ids, out, k)

    w = ActorWorker(cfg.actor_infer, cfg, 0, 1, 0, "actor_infer")
    st = Fake(w)
    st.initialize()
    base = dict(max_new_tokens=4, eos_token_id=[tok.eos_token_id], pad_token_id=tok.pad_token_id, num_beams=1, num_return_sequences=1)
    confs = {100: dict(base, temperature=0.0), 101: dict(base, temperature=1.0, top_k=50, top_p=0.9, seed=3),
             102: dict(base, temperature=0.8, top_k=-1, top_p=0.95, repetition_penalty=1.2), 103: dict(base, temperature=0.0, repetition_penalty=1.3),
             104: dict(base, temperature=0.0), 105: dict(base, temperature=1.0, top_k=2000),
             106: dict(base, temperature=0.0, num_beams=2), 107: dict(base, temperature=0.0, eos_token_id=[9])}
    done = {}
    for rid, gc in confs.items():
        ids = torch.tensor([[1, 2, rid]], dtype=torch.long)
        st.add_request("ADD", DataProto(batch={"input_ids": ids, "attention_mask": torch.ones_like(ids)}, non_tensor_batch={},
                                        meta_info={"request_id": rid, "generation_config": gc}))
    st.add_request("STOP", None)
    st.start_server(data=None, request_complete_callback=lambda data: done.__setitem__(data.meta_info["request_id"], data.meta_info["output_token_ids"]))
    assert sorted(done) == sorted(confs)
    assert sorted(static) == [105, 106, 107]
    adm = [x for x in eng.log if x[0] == "admit"]
    served = sorted(i for x in adm for i in x[1])
    assert served == [100, 101, 102, 103, 104]
    assert sum(1 for x in eng.log if x[0] == "begin") == 1           # ONE batcher served 100-104
    ent = {i: e for x in adm if x[2] is not None for i, e in zip(x[1], x[2])}
    assert ent[101][4] == 3 * 1000003 and ent[101][5] == 0            # its own seed (as generate() derives it), stream = fork
    assert ent[102][3] == pytest.approx(1.2) and ent[103][:4] == (0.0, 1, 1.0, pytest.approx(1.3))
    assert any(x[0] == "step" and x[2] for x in eng.log)
