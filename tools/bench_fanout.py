"""n sampled sequences per prompt from ONE admission (KV prefix fan-out) against n identical n = 1 requests, at the pipeline's stage-1 shape:
two 756 x 756 images per prompt (~1.7 k prompt tokens), the reference YAML's sampling (temperature 1, top_k 100, top_p 0.8), 128 new tokens
(eos ignored), 32 rows, overlapped admission, n = 8 and 32 prompts (256 sequences), SocioReasoner-3B geometry with synthetic weights.
Both runs go through socioreasoner_amd.serving.ContinuousBatcher directly.  A child pass under `rocprofv3 --kernel-trace` times k_kv_fanout
at L = the prompt length, d = n - 1 on the 3B KV geometry and reports the achieved (1 + d) x prefix bytes per second.  Prints one JSON line.

    python tools/bench_fanout.py [--prompts 32] [--n 8] [--no-prof] [--out FILE]
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

GRID = (1, 54, 54)                      # 756 x 756 at patch 14: 2916 patches, 729 merged tokens per image
KVH, LAYERS, CTX = 2, 36, 2048          # SocioReasoner-3B's KV geometry


def kv_bytes_per_token():
    return LAYERS * KVH * 128 * 2 * 2                 # K and V, bf16


def child_kernel(L, d, reps):
    """the fan-out kernel alone on torch-allocated caches (the engine's layout), `reps` launches: the profiled pass"""
    from socioreasoner_amd import lib
    Lb = lib.load()
    S = d + 1
    kc = torch.zeros(LAYERS, S, KVH, CTX, 128, dtype=torch.int16, device="cuda")
    vc = torch.zeros_like(kc)
    dst = torch.arange(1, S, dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(reps + 2):
        if i == 2:
            ev[0].record()
        rc = Lb.sr_op_kv_fanout(C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), LAYERS, S * KVH * CTX * 128, KVH, CTX, 0,
                                C.c_void_p(dst.data_ptr()), d, L, s)
        assert rc == 0
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


def profile_kernel(L, d):
    """rocprofv3 --kernel-trace over a child process that runs the kernel alone -> average k_kv_fanout duration (us)"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found"
    out = tempfile.mkdtemp(prefix="fanout_prof_")
    cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "fanout", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(L), str(d)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return None, f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}"
    import csv
    durs = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "k_kv_fanout" in row.get("Kernel_Name", ""):
                durs.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    shutil.rmtree(out, ignore_errors=True)
    if not durs:
        return None, "no k_kv_fanout dispatch in the trace"
    durs = durs[2:] or durs                          # (the first launches warm up)
    return float(np.median(durs)), f"{len(durs)} dispatches"


def serve(e, reqs, sampling):
    from socioreasoner_amd.serving import ContinuousBatcher
    cb = ContinuousBatcher(e, eos=[], pad_id=0, steps_per_poll=8, sampling=sampling, overlap=True, time_phases=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = cb.run(reqs)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ph = cb.phase_ms()
    adm = sum(v for k, v in ph.items() if k.startswith("vit") or k.startswith("prefill"))
    return out, wall, adm / 1e3, cb.stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, type=int, default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps({"k_kv_fanout_us_events": round(child_kernel(a.child[0], a.child[1], 20), 2)}))
        return
    from socioreasoner_amd import hostops, synthetic
    from socioreasoner_amd.config import geometry_3b
    from socioreasoner_amd.engine import Engine
    from socioreasoner_amd.serving import Request
    g = geometry_3b()
    P, n, R = a.prompts, a.n, a.rows
    ids = [synthetic.tile_prompt(g, i, GRID, n_pre=120, n_post=110, n_images=2) for i in range(P)]
    L = max(len(x) for x in ids)
    pos = [hostops.get_rope_index(torch.from_numpy(x)[None], [GRID, GRID], None)[0][:, 0].numpy() for x in ids]
    ims = [[torch.from_numpy(synthetic.tile_pixels(2 * i + j, 756, 756)).cuda() for j in range(2)] for i in range(P)]
    per_prompt = 2 * GRID[1] * GRID[2]
    e = Engine(g, max_patches=4 * per_prompt, max_prefill_tokens=4 * (L + 64), max_batch=R, max_ctx=(L + a.new + 63) // 64 * 64 + 64,
               max_new_tokens=a.new, kv_slots=2 * R)
    e.load_synthetic_weights(seed=0)
    smp = {"temperature": 1.0, "top_k": 100, "top_p": 0.8, "seed": 1}

    def reqs(fan):
        if fan:
            return [Request(ids=ids[i], pos3=pos[i], max_new=a.new, images=ims[i], grids=[GRID, GRID], n=n) for i in range(P)]
        return [Request(ids=ids[i], pos3=pos[i], max_new=a.new, images=ims[i], grids=[GRID, GRID]) for i in range(P) for _ in range(n)]

    serve(e, reqs(True)[:4], smp)                      # warm-up: graphs captured, the scheduler's share model calibrated
    serve(e, reqs(False)[:4 * n], smp)
    res = {}
    for name, fan in (("fanout", True), ("copies", False), ("fanout_again", True), ("copies_again", False)):
        out, wall, adm_s, st = serve(e, reqs(fan), smp)
        seqs = sum(len(o) for o in out) if fan else len(out)
        assert seqs == P * n
        res[name] = {"seq_per_s": round(seqs / wall, 2), "wall_s": round(wall, 3), "admission_s": round(adm_s, 3),
                     "admission_share": round(adm_s / wall, 4), "admissions": st["admissions"], "admitted_prompts": st["admitted_prompts"],
                     "admitted": st["admitted"]}
    e.close()
    del e
    torch.cuda.empty_cache()
    d = n - 1
    line = {"bench": "fanout_stage1", "prompts": P, "n": n, "rows": R, "new_tokens": a.new, "prompt_tokens": L, "images_per_prompt": 2,
            "image": "756x756", "sampling": smp, "runs": res,
            "speedup_seq_per_s": round(min(res["fanout"]["seq_per_s"], res["fanout_again"]["seq_per_s"])
                                       / max(res["copies"]["seq_per_s"], res["copies_again"]["seq_per_s"]), 3)}
    nbytes = (1 + d) * L * kv_bytes_per_token()
    line["kv_fanout"] = {"L": L, "d": d, "bytes": nbytes}
    if not a.no_prof:
        us, note = profile_kernel(L, d)
        line["kv_fanout"].update({"us_rocprofv3": us, "trace": note})
        if us:
            line["kv_fanout"]["tb_per_s"] = round(nbytes / (us * 1e-6) / 1e12, 3)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(L), str(d)], capture_output=True, text=True, timeout=600)
    if r.returncode == 0 and r.stdout.strip():
        us_ev = json.loads(r.stdout.strip().splitlines()[-1])["k_kv_fanout_us_events"]
        line["kv_fanout"].update({"us_events": us_ev, "tb_per_s_events": round(nbytes / (us_ev * 1e-6) / 1e12, 3)})
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
