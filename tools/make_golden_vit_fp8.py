"""Writes tests/golden/vit_fp8_def3b.npz: the DEFINITION of the fp8 vision tower (sr_config.v_weight_dtype = 2; tests/vit_fp8_ref.py over
oracle/model_ref.py) and the bf16 oracle at full depth -- the 3B tower, one 448 x 448 tile (tile 0 of socioreasoner_amd/synthetic.py),
synthetic weights seed 0 -- on the CPU.  Two forwards of 1.3 TFLOP: minutes, done once.  Kept small: every POOL_STRIDE-th element of both
outputs (the positions tests/golden/hf_truth3b.npz samples, so that the float32 truth there lines up), as bf16 bit patterns, plus
`quant_effect` = rms(definition - bf16 oracle) and the output rms over ALL elements.

    python tools/make_golden_vit_fp8.py [out.npz]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import host_ref as H  # noqa: E402
from oracle import model_ref as MR  # noqa: E402
from oracle import weights as WG  # noqa: E402
from socioreasoner_amd import synthetic  # noqa: E402
from tests.vit_fp8_ref import VitFp8Weights, rms  # noqa: E402

TILE, HW = 0, 448


def bits(x):
    return x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "vit_fp8_def3b.npz")
    truth = np.load(os.path.join(ROOT, "tests", "golden", "hf_truth3b.npz"))
    ps = int(truth["pool_stride"][0])
    assert truth["tile448_tiles"].tolist() == [TILE] and int(truth["tile448_hw"][0]) == HW
    cfg = MR.config_3b()
    W = WG.LazyWeights(cfg, seed=0, fast=True)
    pv, grid = H.patchify(synthetic.tile_pixels(TILE, HW, HW))
    pix = torch.from_numpy(pv)
    t0 = time.time()
    ref = MR.vit_forward(W, cfg, pix, [grid])
    t1 = time.time()
    dfn = MR.vit_forward(VitFp8Weights(W), cfg, pix, [grid])
    t2 = time.time()
    qe, orms = rms(dfn - ref), rms(ref)
    f32 = torch.from_numpy(truth["tile448_pooler_f32"])
    print(f"bf16 oracle {t1 - t0:.0f} s, definition {t2 - t1:.0f} s; quant_effect {qe:.4f}, output rms {orms:.4f}; "
          f"to the float32 truth (strided): bf16 oracle {rms(ref.flatten()[::ps] - f32):.4f}, definition {rms(dfn.flatten()[::ps] - f32):.4f}")
    np.savez_compressed(out_path, tile=np.array([TILE]), hw=np.array([HW]), pool_stride=np.array([ps]), shape=np.array(ref.shape),
                        definition=bits(dfn.flatten()[::ps]), bf16_oracle=bits(ref.flatten()[::ps]),
                        quant_effect=np.array([qe]), output_rms=np.array([orms]))
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
