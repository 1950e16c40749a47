"""The vision tower alone at SocioReasoner-3B shapes with synthetic weights, bf16 (v_weight_dtype 0) against fp8 x fp8 on the block-scaled MFMA
(v_weight_dtype 2, Engine(vit_fp8="mx")): 32 tiles of 448 x 448, 16 tiles of 896 x 896, 16 pairs of 756 x 756 (ragged border windows).
One process, two engines; the modes alternate, three timed windows each per workload (a window = ITERS forwards between two device
synchronisations, after a warm-up of the shape); medians and the spread are reported.  One child pass per mode under
`rocprofv3 --kernel-trace --stats` (no counters in that run) gives the per-kernel time of the 448 workload: GEMM, quantiser, norm, attention.
FLOPs are counted from the shapes (the seven linears + patch embedding; attention excluded from the rate).  Prints one JSON line.

    python tools/bench_vit_fp8.py [--no-prof] [--out FILE]
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

WORKLOADS = {"32x448": (448, 32), "16x896": (896, 16), "16x2x756": (756, 32)}       # name -> (tile side, images in the call)
REPS, ITERS = 3, 3


def engine(mode, max_patches):
    from socioreasoner_amd.config import geometry_3b
    from socioreasoner_amd.engine import Engine
    e = Engine(geometry_3b(), max_patches=max_patches, max_prefill_tokens=64, max_batch=1, max_ctx=64, max_new_tokens=8, vit_fp8="mx" if mode == 2 else False)
    e.load_synthetic_weights(seed=0)
    return e


def pixels(e, hw, n):
    from socioreasoner_amd import synthetic
    one = [e.patchify(torch.from_numpy(synthetic.tile_pixels(i, hw, hw)).cuda()) for i in range(min(n, 4))]
    return torch.cat([one[i % len(one)] for i in range(n)], dim=0), [(1, hw // 14, hw // 14)] * n


def linear_flops(g, n_patches):
    v = g.vision
    C, ip, mh = v.hidden_size, v.intermediate_size, v.hidden_size * v.spatial_merge_size ** 2
    per_patch = v.depth * (3 * C * C + C * C + 3 * C * ip) + (mh * mh + v.out_hidden_size * mh) / v.spatial_merge_size ** 2
    return 2.0 * n_patches * per_patch


def window(e, pix, grids):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        e.vit_forward(pix, grids)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / ITERS


def measure():
    from socioreasoner_amd.config import geometry_3b
    npmax = max((hw // 14) ** 2 * n for hw, n in WORKLOADS.values())
    eng = {0: engine(0, npmax), 2: engine(2, npmax)}
    out = {}
    for name, (hw, n) in WORKLOADS.items():
        pix, grids = pixels(eng[0], hw, n)
        ms = {0: [], 2: []}
        for m in (0, 2):
            eng[m].vit_forward(pix, grids)           # warm-up of the shape (control data, code objects)
        for _ in range(REPS):
            for m in (0, 2):                         # alternating: both modes see the same neighbours on the machine
                ms[m].append(window(eng[m], pix, grids))
        npatch = (hw // 14) ** 2 * n
        fl = linear_flops(geometry_3b(), npatch)
        st = lambda v: {"ms_median": round(float(np.median(v)), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}
        out[name] = {"patches": npatch, "linear_tflop": round(fl / 1e12, 3), "bf16": st(ms[0]), "fp8_mx": st(ms[2]),
                     "speedup_median": round(float(np.median(ms[0]) / np.median(ms[2])), 4),
                     "linear_pflops_whole_tower": {"bf16": round(fl / np.median(ms[0]) / 1e12, 3), "fp8_mx": round(fl / np.median(ms[2]) / 1e12, 3)}}
    for e in eng.values():
        e.close()
    return out


GROUPS = (("gemm_bf16_256", "k_gemm256"), ("gemm_bf16_128", "k_gemm"), ("quant_mx_act", "k_quant_mx_act"), ("rmsnorm_mx", "k_rmsnorm_mx"),
          ("rmsnorm", "k_rmsnorm"), ("attention", "k_attn"))


def classify(kname):
    if "k_gemm256" in kname and ("Lb1" in kname or ", true>" in kname):
        return "gemm_mx"
    for label, key in GROUPS:
        if key in kname:
            return label
    return "other"


def profile(mode):
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"note": "rocprofv3 not found on PATH"}
    out = tempfile.mkdtemp(prefix="vit_fp8_prof_")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "vit", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(mode)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        shutil.rmtree(out, ignore_errors=True)
        return {"note": f"rocprofv3 exit {r.returncode}: {r.stderr[-300:]}"}
    import csv
    us, by_name = {}, {}
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            k = row.get("Kernel_Name", "")
            d = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            us.setdefault(classify(k), []).append(d)
            if "k_gemm256" in k:
                by_name.setdefault(k[:90], []).append(d)
    shutil.rmtree(out, ignore_errors=True)
    total = sum(sum(v) for v in us.values())
    res = {k: {"ms_total": round(sum(v) / 1e3, 3), "share": round(sum(v) / total, 4), "launches": len(v)} for k, v in sorted(us.items())}
    res["gemm256_by_instantiation_ms"] = {k: round(sum(v) / 1e3, 3) for k, v in sorted(by_name.items())}
    res["note"] = "whole child process: engine set-up and weight generation are in `other`; one warm-up and one timed-size forward of 32 x 448"
    return res


def child(mode):
    hw, n = WORKLOADS["32x448"]
    e = engine(mode, (hw // 14) ** 2 * n)
    pix, grids = pixels(e, hw, n)
    e.vit_forward(pix, grids)
    e.vit_forward(pix, grids)
    torch.cuda.synchronize()
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        child(a.child)
        return
    assert torch.cuda.is_available(), "this benchmark measures on the GPU; there is no CPU fallback"
    line = {"bench": "vit_fp8_3b", "reps": REPS, "iters_per_window": ITERS, "workloads": measure()}
    if not a.no_prof:
        line["kernels_rocprofv3_32x448"] = {"bf16": profile(0), "fp8_mx": profile(2)}
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
