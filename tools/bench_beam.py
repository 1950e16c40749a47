"""Beam search on the device (sr_decode_beam) at SocioReasoner-3B shapes with synthetic weights: 8 prompts with one 448 x 448 tile each,
num_beams 4 (32 rows), 128 new tokens (no eos: every run goes the full length).  Reports ms per beam step against a 32-row sampled decode
step (sr_decode_sample) on the same engine, the KV suffix bytes copied per step (from the beam trace), and one run at --long new tokens.
A child pass under `rocprofv3 --kernel-trace --stats` gives the per-launch times of k_beam_rowstats, k_beam_select and k_kv_suffix.
Prints one JSON line.

    python tools/bench_beam.py [--new 128] [--long 1024] [--no-prof] [--out FILE]
"""
import argparse
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

GRID = (1, 32, 32)                      # 448 x 448 at patch 14: 1024 patches, 256 merged tokens
KVH, LAYERS = 2, 36
KV_BYTES_PER_POS = LAYERS * KVH * 128 * 2 * 2          # K and V, bf16, all layers
G, W = 8, 4


def setup(new):
    from socioreasoner_amd import hostops, synthetic
    from socioreasoner_amd.config import geometry_3b
    from socioreasoner_amd.engine import Engine
    g = geometry_3b()
    ids = [synthetic.tile_prompt(g, i, GRID, n_pre=120, n_post=110, n_images=1) for i in range(G)]
    pos = [hostops.get_rope_index(torch.from_numpy(x)[None], [GRID], None)[0][:, 0].numpy() for x in ids]
    L = max(len(x) for x in ids)
    e = Engine(g, max_patches=G * GRID[1] * GRID[2], max_prefill_tokens=W * G * (L + 8), max_batch=G * W,
               max_ctx=(L + new + 63) // 64 * 64 + 64, max_new_tokens=new)
    e.load_synthetic_weights(seed=0)
    pix = torch.cat([e.patchify(torch.from_numpy(synthetic.tile_pixels(i, 448, 448)).cuda()) for i in range(G)], dim=0)
    emb = e.vit_forward(pix, [GRID] * G)
    return e, ids, pos, emb, L


def beam_run(e, ids, pos, emb, new, trace=False):
    e.prefill(ids, pos, emb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.decode_beam(W, new, 1, 1.0, eos=[], pad_id=0, trace=trace)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e.steps_done


def sample_run(e, ids, pos, emb, new):
    rep = [x for x in ids for _ in range(W)]
    rp = [p for p in pos for _ in range(W)]
    erep = torch.cat([emb.view(G, -1, emb.shape[-1])[i] for i in range(G) for _ in range(W)], dim=0)
    e.prefill(rep, rp, erep)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.decode_sample(new, 1.0, 100, 0.8, seed=1, eos=[], pad_id=0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e.steps_done


def copied_bytes(e, steps):
    """KV suffix bytes copied per step: every child beyond a parent's first copies positions [prompt, ctx) = t generated positions"""
    tr = e.beam_trace.cpu()[:steps]
    per = []
    for t in range(1, steps):
        n = 0
        for g in range(G):
            par = tr[t, g * W:(g + 1) * W, 0].tolist()
            if par[0] >= 0:
                n += W - len(set(par))
        per.append(n * t * KV_BYTES_PER_POS)
    return float(np.mean(per)) if per else 0.0, float(max(per)) if per else 0.0


def measure(new):
    e, ids, pos, emb, L = setup(new)
    beam_run(e, ids, pos, emb, min(new, 32))        # warm-up: graphs captured
    sample_run(e, ids, pos, emb, min(new, 32))
    bms, bsteps = min(beam_run(e, ids, pos, emb, new) for _ in range(2))
    sms, ssteps = min(sample_run(e, ids, pos, emb, new) for _ in range(2))
    beam_run(e, ids, pos, emb, new, trace=True)
    mean_b, max_b = copied_bytes(e, e.steps_done)
    e.close()
    return {"prompt_tokens": L, "beam_ms_per_step": round(bms / bsteps, 4), "sample_ms_per_step": round(sms / ssteps, 4),
            "beam_over_sample": round((bms / bsteps) / (sms / ssteps), 4), "steps": bsteps,
            "suffix_bytes_per_step_mean": int(mean_b), "suffix_bytes_per_step_max": int(max_b)}


def profile(new):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return {"note": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="beam_prof_")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "beam", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(new)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        shutil.rmtree(out, ignore_errors=True)
        return {"note": f"rocprofv3 exit {r.returncode}: {r.stderr[-300:]}"}
    import csv
    durs = {"k_beam_rowstats": [], "k_beam_select": [], "k_kv_suffix": []}
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            for k in durs:
                if k in row.get("Kernel_Name", ""):
                    durs[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    shutil.rmtree(out, ignore_errors=True)
    return {k: {"us_median": round(float(np.median(v)), 2), "us_mean": round(float(np.mean(v)), 2), "launches": len(v)} for k, v in durs.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--long", type=int, default=1024)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child:                                      # the profiled pass: one beam run (graph replay)
        e, ids, pos, emb, _ = setup(a.child)
        beam_run(e, ids, pos, emb, a.child)
        e.close()
        return
    line = {"bench": "beam_3b", "prompts": G, "num_beams": W, "rows": G * W, "image": "448x448", "runs": {str(a.new): measure(a.new)}}
    if a.long:
        line["runs"][str(a.long)] = measure(a.long)
    if not a.no_prof:
        line["kernels_rocprofv3"] = profile(a.new)
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
