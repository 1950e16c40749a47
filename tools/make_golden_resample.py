"""Writes tests/golden/pil_resample.npz: inputs and Pillow's own outputs of the small resampling cases that tests/test_host_resample.py and
tests/test_gpu_resample.py hold hostops.pil_resize_ref and raster.resize_pil to, so that those tests do not depend on the Pillow version of the
machine they run on (the larger cases are compared with the installed Pillow only: noise does not compress and the file stays under 200 KB).

    python tools/make_golden_resample.py

Keys: "<h>x<w>_<noise|edge>_in" (uint8 [h, w, 3]; the 1-channel cases take its channel 0), "<h>x<w>_<H>x<W>_c<channels>_<noise|edge>_<filter>_out",
"pillow_version"."""
from __future__ import annotations

import os
import sys

import numpy as np
from PIL import Image
import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pil_resample.npz")

# (h, w) -> (H, W): odd sizes whose rows are neither dword-aligned nor a multiple of 4 bytes long, both directions, one-pass resizes
SMALL_CASES = [((37, 53), (28, 56)), ((53, 37), (84, 28)), ((5, 7), (28, 28)), ((64, 64), (64, 28)), ((64, 64), (28, 64))]
FILTERS = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "lanczos": Image.LANCZOS}


def case_name(hw, HW, c, kind):
    return f"{hw[0]}x{hw[1]}_{HW[0]}x{HW[1]}_c{c}_{kind}"


def input_name(hw, kind):
    return f"{hw[0]}x{hw[1]}_{kind}_in"


def make_input(hw, kind):
    """uint8 [h, w, 3], seeded by the size.  noise: uniform bytes; edge: 0 / 255 only (every overshoot of the negative lobes clips)."""
    rng = np.random.default_rng(1000 * hw[0] + hw[1])
    if kind == "noise":
        return rng.integers(0, 256, hw + (3,), dtype=np.uint8)
    return (rng.integers(0, 2, hw + (3,), dtype=np.uint8) * 255).astype(np.uint8)


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for hw, HW in SMALL_CASES:
        for kind in ("noise", "edge"):
            x3 = out.setdefault(input_name(hw, kind), make_input(hw, kind))
            for c in (3, 1):
                x = x3 if c == 3 else np.ascontiguousarray(x3[:, :, 0])
                for f, pf in FILTERS.items():
                    if c == 1 and f != "bicubic":
                        continue
                    out[f"{case_name(hw, HW, c, kind)}_{f}_out"] = np.asarray(Image.fromarray(x).resize((HW[1], HW[0]), resample=pf))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays, Pillow", PIL.__version__)


if __name__ == "__main__":
    sys.exit(main())
