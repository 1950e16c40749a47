"""CPU tests of num_return_sequences n > 1 through the host layers: the generate scheduler passes n to the worker at both levels (no prompt copies)
and lays the answers out prompt-major with a prompt's n rows adjacent; the cross-rank dispatcher carries n lists per request and counts n sequences
per request against max_running_requests."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_worker(tmp_path, n, expand, level):
    from roll.distributed.strategy.mi355x_strategy import Mi355xStrategy
    from roll.pipeline.base_worker import ActorWorker
    from socioreasoner_amd import hostops
    from socioreasoner_amd.config import geometry_tiny
    from socioreasoner_amd.textproc import ByteTokenizer
    from tests.test_host_cpu import _tiny_cfg
    cfg = _tiny_cfg(tmp_path, prompt_length=12, response_length=6)
    cfg.actor_infer.generating_args["num_return_sequences"] = n
    cfg["is_num_return_sequences_expand"] = expand
    cfg["generate_opt_level"] = level
    tok = ByteTokenizer(geometry_tiny())
    calls = []

    class Fake(Mi355xStrategy):          # the real request loop (start_server / add_request), a scripted engine: answer j of a prompt names j
        max_batch = 2

        def initialize(self, model_provider=None):
            import queue
            self.command_queue, self.tokenizer = queue.Queue(), tok

        def generate(self, batch, generation_config):
            ids, mask = batch.batch["input_ids"], batch.batch["attention_mask"]
            k = int(generation_config["num_return_sequences"])
            calls.append((len(ids), k))
            rows = []
            for r, m in zip(ids, mask):
                p = r[m.bool()].tolist()
                for j in range(k):
                    rows.append([p[-1], 100 + j] + [tok.eos_token_id])
            out = hostops.gather_outputs_to_pad_tensor(rows, generation_config["pad_token_id"], device=ids.device)
            return hostops.concatenate_input_and_output(ids, out, k)

    w = ActorWorker(cfg.actor_infer, cfg, 0, 1, 0, "actor_infer")
    w.strategy = Fake(w)
    w.strategy.initialize()
    w.tokenizer = tok
    return w, cfg, calls, tok


def _batch(B=5, P=12):
    from roll.distributed.scheduler.protocol import DataProto
    rng = np.random.default_rng(0)
    ids = torch.full((B, P), 0, dtype=torch.long)
    mask = torch.zeros(B, P, dtype=torch.long)
    for i, k in enumerate([12, 7, 9, 3, 10][:B]):
        ids[i, P - k:] = torch.from_numpy(rng.integers(0, 250, k))
        mask[i, P - k:] = 1
    pos = (mask.cumsum(-1) - 1).clamp(min=0)[:, None, :].repeat(1, 3, 1)
    return DataProto(batch={"input_ids": ids, "attention_mask": mask, "position_ids": pos}, non_tensor_batch={}), ids


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("expand", [False, True])
def test_generate_scheduler_passes_n_and_returns_n_rows_per_prompt(tmp_path, level, expand):
    """Both levels, is_num_return_sequences_expand on and off: the worker is asked for n = 3 sequences of each of the B prompts (never for copies
    of a prompt), and the output has B x 3 rows -- prompt-major, a prompt's three answers adjacent in fork order, each row carrying its prompt:
    the layout the expanded batch had.  Level 1 used to drop n (one row per prompt)."""
    from roll.distributed.scheduler.generate_scheduler import GenerateScheduler
    n, B = 3, 5
    w, cfg, calls, tok = _fake_worker(tmp_path, n, expand, level)
    data, ids = _batch(B)
    out = GenerateScheduler().generate(data, w, cfg)
    assert calls and all(k == n for _, k in calls), calls
    assert sum(b for b, _ in calls) == B, calls                      # every prompt once
    resp = out.batch["responses"]
    assert resp.shape[0] == B * n and out.batch["prompts"].shape[0] == B * n
    assert torch.equal(out.batch["prompts"], ids.repeat_interleave(n, dim=0))
    for i in range(B):
        for j in range(n):
            assert resp[i * n + j, :2].tolist() == [int(ids[i, -1]), 100 + j], (i, j, resp[i * n + j].tolist())


def test_level0_and_level1_agree_with_n(tmp_path):
    from roll.distributed.scheduler.generate_scheduler import GenerateScheduler
    outs = []
    for level in (0, 1):
        w, cfg, _, _ = _fake_worker(tmp_path, 2, False, level)
        data, _ = _batch(4)
        outs.append(GenerateScheduler().generate(data, w, cfg))
    for k in outs[0].batch:
        assert torch.equal(outs[0].batch[k], outs[1].batch[k]), k


def test_assemble_responses_takes_n(tmp_path):
    from roll.distributed.scheduler.generate_scheduler import assemble_responses
    w, cfg, _, tok = _fake_worker(tmp_path, 2, False, 0)
    data, ids = _batch(3)
    rows = [[7, 8, tok.eos_token_id], [9, tok.eos_token_id]] * 3
    out = assemble_responses(data, rows, w, cfg, 2)
    assert out.batch["responses"].shape[0] == 6 and torch.equal(out.batch["prompts"], ids.repeat_interleave(2, dim=0))
    with pytest.raises(AssertionError):
        assemble_responses(data, rows[:3], w, cfg, 2)


_FANOUT_DISPATCH_WORKER = r"""
import os, sys, time, queue
import numpy as np, torch
sys.path.insert(0, {root!r})
from socioreasoner_amd import dp
from socioreasoner_amd.dispatch import CrossRankDispatcher, default_store

rank, world, _ = dp.init_distributed("gloo")
N = 2
# a scripted request loop: a request's answers are (gid, fork) pairs, reported after a short delay; in-flight SEQUENCES are tracked per rank
inbox = queue.Queue()
state = {{"sink": None, "running": 0, "peak": 0}}


def add_request(req):
    state["running"] += N
    state["peak"] = max(state["peak"], state["running"])
    inbox.put(req)


def serve():
    while True:
        req = inbox.get()
        if req is None:
            return
        time.sleep(0.01)
        gid = int(req.meta_info["request_id"])
        state["running"] -= N
        state["sink"](gid, [[gid, j] for j in range(N)])


class Req:
    def __init__(self, batch, non_tensor_batch, meta_info):
        self.batch, self.non_tensor_batch, self.meta_info = batch, non_tensor_batch, meta_info


t = __import__("threading").Thread(target=serve, daemon=True)
t.start()
sizes = [5, 3]
mine = [Req({{"x": torch.tensor([rank, i])}}, {{}}, {{}}) for i in range(sizes[rank])]
# cap 4 sequences = two requests of n = 2 per worker
d = CrossRankDispatcher(default_store(), rank, world, round_id=7, max_running_requests=4, timeout_s=60.0, num_return_sequences=N)
got = d.run(mine, add_request=add_request, make_result_sink=lambda cb: state.__setitem__("sink", cb),
            make_request=lambda b, n, m: Req(b, n, m))
inbox.put(None)
off = sum(sizes[:rank])
assert sorted(got) == list(range(sizes[rank])), got
for i in range(sizes[rank]):
    assert got[i] == [[off + i, 0], [off + i, 1]], (rank, i, got[i])
assert state["peak"] <= 4, state
dp.barrier()
print("ok", rank, d.stats)
"""


def test_cross_rank_dispatcher_carries_n_lists_two_ranks_gloo(tmp_path):
    """A 2-rank gloo run of the cross-rank dispatcher with num_return_sequences 2: every rank gets the two token lists of each of its own
    requests back (whoever served them), and no worker ever has more than max_running_requests sequences in flight (a request counts as 2)."""
    script = tmp_path / "w.py"
    script.write_text(_FANOUT_DISPATCH_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29553")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29553", str(script)],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("ok") == 2
