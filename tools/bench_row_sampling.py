"""Per-request sampling in the continuous batcher at SocioReasoner-3B shapes (synthetic weights, 32 rows, text prompts of 400-480 tokens):
  1. ms per decode step (device events over 64 replays): the shared sampled step (sr_rows_sampling) against the per-row step with a uniform
     table and with a mixed table (a quarter each greedy, top-k 100 / top-p 0.8, unbounded nucleus top-p 0.9, top-k 100 with penalty 1.05);
  2. k_sample on 32 penalised rows (rp 1.05, top_k 100, the prompt + 128 tokens seen) of the 3B engine's own logits: with the LM head's block
     maxima (the penalty-aware shortcut) against the full-vocabulary scan (sr_op_sample without maxima), device events over 200 launches;
  3. a stream of 96 requests alternating two sampling configurations (64 new tokens each): one batcher, the second configuration as the
     requests' own parameters (this version), against the previous version's handling -- the first configuration's requests in the batcher,
     the other's waiting for them to drain and then served by the static path (prefill + sr_decode_sample per batch of 32).
A child pass under `rocprofv3 --kernel-trace --stats` runs the mixed-table steps and the two sampler forms: per-launch k_sample* times.
Prints one JSON line.

    python tools/bench_row_sampling.py [--no-prof] [--out FILE]
"""
import argparse
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MB, NEW = 32, 64
A = {"temperature": 1.0, "top_k": 100, "top_p": 0.8, "seed": 1}
BCONF = {"temperature": 0.7, "top_k": 20, "top_p": 0.95}
MIXED = [(0.0, 1, 1.0, 1.0), (1.0, 100, 0.8, 1.0), (1.0, -1, 0.9, 1.0), (1.0, 100, 0.8, 1.05)]


def setup():
    from socioreasoner_amd.config import geometry_3b
    from socioreasoner_amd.engine import Engine
    g = geometry_3b()
    rng = np.random.default_rng(0)
    ids = [rng.integers(0, 150000, int(rng.integers(400, 480))).astype(np.int64) for _ in range(96)]
    pos = [np.tile(np.arange(len(x)), (3, 1)).astype(np.int64) for x in ids]
    e = Engine(g, max_patches=64, max_prefill_tokens=MB * 480, max_batch=MB, max_ctx=1024, max_new_tokens=256, kv_slots=2 * MB)
    e.load_synthetic_weights(seed=0)
    return e, ids, pos


def steps(e, ids, pos, mode, n=64):
    """ms per step of n replays after 8 warm-up steps, 32 rows admitted at once"""
    e.rows_begin()
    sampling = None
    if mode == "shared":
        e.rows_sampling(A["temperature"], A["top_k"], A["top_p"], A["seed"])
    elif mode == "uniform":
        e.rows_sampling(A["temperature"], A["top_k"], A["top_p"], A["seed"])
        e.rows_per_row(True)
    else:
        e.rows_per_row(True)
        sampling = [MIXED[j % 4] + (7, j) for j in range(MB)]
    e.admit(list(range(MB)), ids[:MB], pos[:MB], [n + 16] * MB, sampling=sampling)
    e.rows_step(8)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    e.rows_step(n)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def sampler(e, ids, pos, launches=200):
    """k_sample on the engine's own logits with 32 penalised rows: block maxima (shortcut) against none (full scan)"""
    from socioreasoner_amd import lib
    L = lib.load()
    V = e.geom.text.vocab_size
    e.rows_begin()
    logits = e.admit(list(range(MB)), ids[:MB], pos[:MB], [2] * MB, return_logits=True)
    R = 64
    nb = (V + R - 1) // R
    pad = torch.full((MB, nb * R), float("-inf"), device="cuda")
    pad[:, :V] = logits
    bmax = pad.view(MB, nb, R).amax(-1).contiguous()
    seen = torch.zeros(MB, V, dtype=torch.bool, device="cuda")
    rng = np.random.default_rng(1)
    for r in range(MB):
        seen[r, torch.from_numpy(ids[r]).cuda()] = True
        seen[r, torch.from_numpy(rng.integers(0, V, 128)).cuda()] = True
    W = (V + 31) // 32
    bits = torch.zeros(MB, W * 32, dtype=torch.int64, device="cuda")
    bits[:, :V] = seen.long()
    w = (bits.view(MB, W, 32) << torch.arange(32, device="cuda")).sum(-1)
    words = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()
    step = torch.zeros(MB, dtype=torch.int32, device="cuda")
    out = {k: torch.empty(MB, dtype=torch.int64, device="cuda") for k in ("shortcut", "full")}
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for name, bm in (("shortcut", bmax), ("full", None)):
        def go():
            rc = L.sr_op_sample(C.c_void_p(logits.data_ptr()), MB, V, 1.0, 100, 0.8, 1.05, C.c_void_p(words.data_ptr()), 3, C.c_void_p(step.data_ptr()),
                                C.c_void_p(out[name].data_ptr()), C.c_void_p(bm.data_ptr()) if bm is not None else None, nb, R, s)
            assert rc == 0, L.sr_last_error(None)
        for _ in range(10):
            go()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            go()
        b.record()
        torch.cuda.synchronize()
        res[name + "_us"] = round(a.elapsed_time(b) * 1e3 / launches, 2)
    res["same_tokens"] = bool(torch.equal(out["shortcut"], out["full"]))
    return res


def stream(e, ids, pos, before):
    """96 requests alternating A / B, 64 new tokens each, no eos -> sequences per second"""
    from socioreasoner_amd.serving import ContinuousBatcher, Request
    reqs = [Request(ids=ids[k], pos3=pos[k], max_new=NEW, sampling=None if k % 2 == 0 else dict(BCONF)) for k in range(96)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if before:          # previous version: B waits until the batcher drains, then static batches of 32 (prefill + sr_decode_sample)
        cb = ContinuousBatcher(e, eos=[], pad_id=0, sampling=A, overlap=True)
        cb.run([r for r in reqs if r.sampling is None])
        cb._hand_back()
        rest = [r for r in reqs if r.sampling is not None]
        for c in range(0, len(rest), MB):
            grp = rest[c:c + MB]
            e.prefill([r.ids for r in grp], [r.pos3 for r in grp])
            e.decode_sample(NEW, BCONF["temperature"], BCONF["top_k"], BCONF["top_p"], 1.0, 104729 * c + 1)
    else:
        cb = ContinuousBatcher(e, eos=[], pad_id=0, sampling=A, overlap=True)
        cb.run(reqs)
        cb._hand_back()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"s": round(dt, 3), "sequences_per_s": round(96 / dt, 2)}


def profile():
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return {"note": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="rowsmp_prof_")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "rowsmp", "--", sys.executable, os.path.abspath(__file__), "--child"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        shutil.rmtree(out, ignore_errors=True)
        return {"note": f"rocprofv3 exit {r.returncode}: {r.stderr[-300:]}"}
    import csv
    durs = {}
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            k = row.get("Kernel_Name", "")
            for name in ("k_sample_full", "k_sample", "k_mark_rows", "k_mark_staged"):
                if name + "(" in k or k.endswith(name) or (name + " ") in k or k.startswith(name):
                    durs.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
                    break
    shutil.rmtree(out, ignore_errors=True)
    return {k: {"us_median": round(float(np.median(v)), 2), "us_mean": round(float(np.mean(v)), 2), "launches": len(v)} for k, v in durs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    e, ids, pos = setup()
    if a.child:                                     # the profiled pass: mixed-table steps and the two sampler forms
        steps(e, ids, pos, "mixed", 32)
        sampler(e, ids, pos, 50)
        e.close()
        return
    line = {"bench": "row_sampling_3b", "rows": MB, "prompt_tokens": "400-480", "mixed_table": MIXED}
    for mode in ("shared", "uniform", "mixed", "shared", "uniform", "mixed"):      # alternated, two rounds
        line.setdefault("step_ms", {}).setdefault(mode, []).append(round(steps(e, ids, pos, mode), 4))
    line["k_sample_penalised_32_rows"] = sampler(e, ids, pos)
    stream(e, ids, pos, False)                      # warm-up (graphs, calibration)
    line["alternating_stream"] = {"after": [stream(e, ids, pos, False) for _ in range(2)], "before_emulated": [stream(e, ids, pos, True) for _ in range(2)]}
    e.close()
    if not a.no_prof:
        line["kernels_rocprofv3"] = profile()
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
