"""What recording token log-probs (sr_logprobs) costs per decode step at SocioReasoner-3B shapes (synthetic weights, text prompts of 448 tokens,
rows admitted once and decoded for up to 500 tokens):
  1. ms per decode step (device events over windows of 20 replays) with the switch off / N = 0 / N = 8, for the shared greedy step, the shared
     sampled step and the per-row step, at 32 and at 128 rows.  The three modes alternate over WINDOWS windows of the same running rows (the
     switch may change between any two steps), so drift -- the context grows -- hits all modes alike; every window's figure is reported.
  2. a child pass under `rocprofv3 --kernel-trace --stats`: per-launch times of the two log-prob kernels against the B x V x 4 bytes of
     logits they read, as a share of the HBM rate (8 TB/s peak).  The kernels read every logit once and do a few flops per element: the
     bound is bandwidth.
Prints one JSON line.

    python tools/bench_logprobs.py [--no-prof] [--rows 32,128] [--out FILE]
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT, WINDOWS, WIN_STEPS, WARM = 448, 5, 20, 2
MODES = (("off", None), ("n0", 0), ("n8", 8))
KINDS = ("greedy", "sampled", "per_row")
HBM_PEAK = 8.0e12


def setup(MB):
    from socioreasoner_amd.config import geometry_3b
    from socioreasoner_amd.engine import Engine
    g = geometry_3b()
    rng = np.random.default_rng(0)
    ids = [rng.integers(0, 150000, PROMPT).astype(np.int64) for _ in range(MB)]
    pos = [np.tile(np.arange(PROMPT), (3, 1)).astype(np.int64) for _ in ids]
    e = Engine(g, max_patches=64, max_prefill_tokens=32 * PROMPT, max_batch=MB, max_ctx=1024, max_new_tokens=512)
    e.load_synthetic_weights(seed=0)
    return e, ids, pos


def start_rows(e, ids, pos, kind):
    """all rows admitted (32 at a time), running under the step of `kind`"""
    MB = e.cfg.max_batch
    e.logprobs(None)
    e.rows_begin()
    if kind == "sampled":
        e.rows_sampling(1.0, 50, 0.9, 1)
    if kind == "per_row":
        e.rows_per_row(True)
    for r0 in range(0, MB, 32):
        rows = list(range(r0, min(r0 + 32, MB)))
        smp = [((0.0, 1, 1.0, 1.0), (1.0, 100, 0.8, 1.0), (1.0, -1, 0.9, 1.0), (1.0, 100, 0.8, 1.05))[j % 4] + (7, j) for j in rows] if kind == "per_row" else None
        e.admit(rows, [ids[r] for r in rows], [pos[r] for r in rows], [500] * len(rows), sampling=smp)


def window(e, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    e.rows_step(n)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def step_times(e, ids, pos, kind):
    """{mode: [ms per step of every window]} with the modes alternating over the windows of one set of running rows"""
    start_rows(e, ids, pos, kind)
    out = {name: [] for name, _ in MODES}
    for _ in range(WINDOWS):
        for name, n in MODES:
            e.logprobs(n)
            e.rows_step(WARM)              # (a switch captures the step again: outside the window)
            torch.cuda.synchronize()
            out[name].append(round(window(e, WIN_STEPS), 4))
    e.logprobs(None)
    return out


def summary(t):
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {"windows_ms": t, "median_ms": {k: round(v, 4) for k, v in med.items()},
            "spread_ms": {k: round(max(v) - min(v), 4) for k, v in t.items()},
            "added_us_vs_off": {k: round((med[k] - med["off"]) * 1e3, 1) for k in med if k != "off"}}


def profile(MB):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return {"note": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="lp_prof_")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "lp", "--", sys.executable, os.path.abspath(__file__), "--child",
           "--rows", str(MB)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        shutil.rmtree(out, ignore_errors=True)
        return {"note": f"rocprofv3 exit {r.returncode}: {r.stderr[-300:]}"}
    import csv
    durs = {}
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            k = row.get("Kernel_Name", "")
            for name in ("k_lp_parts", "k_lp_finish"):
                if name in k:
                    durs.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    shutil.rmtree(out, ignore_errors=True)
    res = {k: {"us_median": round(float(np.median(v)), 2), "us_mean": round(float(np.mean(v)), 2), "launches": len(v)} for k, v in durs.items()}
    if "k_lp_parts" in res:          # (the child runs N = 8 only: the chunk pass with its eight selection rounds)
        nbytes = MB * 151936 * 4
        rate = nbytes / (res["k_lp_parts"]["us_median"] * 1e-6)
        res["logits_bytes"] = nbytes
        res["k_lp_parts_GBps"] = round(rate / 1e9, 1)
        res["k_lp_parts_share_of_hbm_peak"] = round(rate / HBM_PEAK, 3)
        res["bound"] = ("bandwidth: every logit is read once, a few flops per element (the floor is logits_bytes / HBM rate); what the kernels lose "
                        "against it is latency -- the selection rounds of the chunk pass and of the finish")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--rows", default="32,128")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    rows = [int(x) for x in a.rows.split(",")]
    if a.child:                                     # the profiled pass: greedy steps recording N = 8
        e, ids, pos = setup(rows[0])
        start_rows(e, ids, pos, "greedy")
        e.logprobs(8)
        e.rows_step(40)
        torch.cuda.synchronize()
        e.close()
        return
    line = {"bench": "logprobs_3b", "prompt_tokens": PROMPT, "window_steps": WIN_STEPS, "windows": WINDOWS, "rows": {}}
    for MB in rows:
        e, ids, pos = setup(MB)
        line["rows"][str(MB)] = {kind: summary(step_times(e, ids, pos, kind)) for kind in KINDS}
        e.close()
        del e
        if not a.no_prof:
            line["rows"][str(MB)]["kernels_rocprofv3"] = profile(MB)
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
