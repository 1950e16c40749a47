"""The resize in front of the ViT / SAM2, 768 x 768 -> 756 x 756 RGB (the SocioSeg tile under smart_resize), host against device on one MI355X:

  host    PIL bicubic on the calling thread + upload of the 756 x 756 result            (device_resize: false)
  device  upload of the 768 x 768 source + raster.resize_pil (sr_resize_pil_u8)         (device_resize: true)

per image and for a batch of 16 (host: 16 x (PIL + upload); device: 16 x (upload + resize), as Mi355xStrategy._prepare issues them, and
"device_stacked": one upload of [16, 768, 768, 3] + one resize call, as a caller that holds a batch could).  The two sides alternate in one
session, WINDOWS windows each, a window = ITERS repetitions between two device synchronisations after a warm-up; medians and the spread
(min - max) are reported, and `default_stands` says whether the device path's median is faster than the host's by more than the larger spread.
Each kernel alone: its pass through the C ABI (a width-only / height-only resize runs exactly one kernel), KERNEL_ITERS back-to-back launches between
two device events, against the bytes the pass has to move (source read once + destination written once) at the HBM rate.  The outputs of the two
sides are compared byte for byte before anything is timed.  Prints one JSON line; --out FILE also writes it.

    python tools/bench_resize.py [--out profiles/device_resize.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SRC, DST, BATCH = 768, 756, 16
WINDOWS, ITERS, ITERS_BATCH, KERNEL_ITERS = 7, 40, 4, 200
HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.29          # spec; measured float4 copy


def host_path(arrs):
    from PIL import Image
    out = []
    for a in arrs:
        r = np.asarray(Image.fromarray(a).resize((DST, DST), resample=Image.BICUBIC))
        out.append(torch.from_numpy(np.array(r, dtype=np.uint8, order="C")).cuda())
    return out


def device_path(arrs):
    from socioreasoner_amd import raster
    return [raster.resize_pil(torch.from_numpy(a).cuda(), DST, DST, "bicubic") for a in arrs]


def device_stacked(stack):
    from socioreasoner_amd import raster
    return raster.resize_pil(torch.from_numpy(stack).cuda(), DST, DST, "bicubic")


def window(fn, arg, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn(arg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def stat(v):
    return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "windows": len(v)}


def kernel_alone(n_img):
    """-> per pass: µs per launch, bytes, share of the HBM rate."""
    from socioreasoner_amd import raster
    out = {}
    rng = np.random.default_rng(1)
    for name, (h, w, H, W) in {"k_resample_h": (SRC, SRC, SRC, DST), "k_resample_v": (SRC, DST, DST, DST)}.items():
        x = torch.from_numpy(rng.integers(0, 256, (n_img, h, w, 3), dtype=np.uint8)).cuda()
        for _ in range(3):
            raster.resize_pil(x, H, W)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        us = []
        for _ in range(3):
            torch.cuda.synchronize()
            a.record()
            for _ in range(KERNEL_ITERS):
                raster.resize_pil(x, H, W)
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / KERNEL_ITERS)
        nbytes = n_img * 3 * (h * w + H * W)
        t = float(np.median(us))
        out[name] = {"shape": f"{n_img} x {h}x{w} -> {H}x{W} RGB", "us_per_launch_median": round(t, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                     "bytes": nbytes, "us_at_hbm_spec": round(nbytes / HBM_PEAK_TBS / 1e6, 3), "us_at_hbm_measured_copy": round(nbytes / HBM_COPY_TBS / 1e6, 3),
                     "share_of_hbm_spec": round(nbytes / HBM_PEAK_TBS / 1e6 / t, 4),
                     "note": "back-to-back launches through raster.resize_pil between two device events: the host's launch rate bounds it from below"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize.py measures on the GPU: no device found")
    import PIL
    rng = np.random.default_rng(0)
    arrs = [rng.integers(0, 256, (SRC, SRC, 3), dtype=np.uint8) for _ in range(BATCH)]
    stack = np.stack(arrs)
    # same pixels first
    h, d, s = host_path(arrs), device_path(arrs), device_stacked(stack)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(h, d)) and all(torch.equal(s[i], h[i]) for i in range(BATCH))
    if not same:
        raise SystemExit("device resize differs from PIL: nothing timed")
    res = {"workload": f"{SRC}x{SRC} -> {DST}x{DST} RGB, bicubic", "pillow": PIL.__version__, "device": torch.cuda.get_device_name(0), "identical_pixels": same}
    one = {"host": [], "device": []}
    for fn, key in ((host_path, "host"), (device_path, "device")):
        window(fn, arrs[:1], 5)
    for _ in range(WINDOWS):
        for fn, key in ((host_path, "host"), (device_path, "device")):          # alternating
            one[key].append(window(fn, arrs[:1], ITERS))
    bat = {"host": [], "device": [], "device_stacked": []}
    sides = ((host_path, "host", arrs), (device_path, "device", arrs), (device_stacked, "device_stacked", stack))
    for fn, key, arg in sides:
        window(fn, arg, 1)
    for _ in range(WINDOWS):
        for fn, key, arg in sides:
            bat[key].append(window(fn, arg, ITERS_BATCH) / BATCH)

    def verdict(v):
        spread = max(max(v["host"]) - min(v["host"]), max(v["device"]) - min(v["device"]))
        gain = float(np.median(v["host"]) - np.median(v["device"]))
        return {"host_minus_device_ms": round(gain, 4), "largest_spread_ms": round(spread, 4), "device_faster_by_more_than_the_spread": bool(gain > spread)}
    res["per_image"] = {k: stat(v) for k, v in one.items()} | verdict(one)
    res[f"batch_of_{BATCH}_per_image"] = {k: stat(v) for k, v in bat.items()} | verdict(bat)
    res["default_stands"] = bool(res["per_image"]["device_faster_by_more_than_the_spread"] and res[f"batch_of_{BATCH}_per_image"]["device_faster_by_more_than_the_spread"])
    res["kernels_alone_1_image"] = kernel_alone(1)
    res[f"kernels_alone_{BATCH}_images"] = kernel_alone(BATCH)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
