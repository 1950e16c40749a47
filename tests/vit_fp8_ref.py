"""The definition of the fp8 vision tower (sr_config.v_weight_dtype = 2; include/socior.h) as a weight view: handed to ``oracle.model_ref.vit_forward``
it makes that function the definition, without touching the oracle -- ``MR.linear`` applies ``QuantW`` (fp8 e4m3 weights, one float32 scale per
output channel) and ``mx_act`` (the input MX-quantised after its bf16 rounding) generically.  Also the two small geometries and the two images
the GPU tests and the host tests share."""
import re

import torch

from oracle import model_ref as MR

# the seven linears the mode covers; the patch embedding, norm weights and every bias pass through
VIT_FP8 = re.compile(r"visual\.(blocks\.\d+\.(attn\.(qkv|proj)|mlp\.(gate|up|down)_proj)|merger\.mlp\.[02])\.weight$")


class VitFp8Weights:
    """View of a weight mapping (``oracle.weights.LazyWeights``) in which the vision tower's linears are ``QuantW`` with ``mx_act``."""

    def __init__(self, base):
        self.base, self._cache = base, {}

    def __getitem__(self, name):
        if VIT_FP8.match(name):
            if name not in self._cache:
                q = MR.QuantW(self.base[name])
                q.mx_act = True
                self._cache[name] = q
            return self._cache[name]
        return self.base[name]

    def __contains__(self, name):
        return name in self.base


def _tiny_text():
    return dict(num_hidden_layers=3, hidden_size=512, num_attention_heads=4, num_key_value_heads=1, intermediate_size=1000, vocab_size=2048)


def small_configs(name):
    """(oracle RefConfig, engine ModelGeometry) of one of the two small towers the mode can run, over the tiny LM:
    small128: head_dim 128, every width the smallest the kernels take (K = 256: two k-tiles);  true80: the 3B tower's widths (head_dim 80,
    K = 1280 / 3456 / 5120 with the odd k-tile count) at depth 2.  Block 0 is windowed attention, block 1 full attention."""
    from socioreasoner_amd.config import ModelGeometry, TextGeometry, VisionGeometry
    v = {"small128": dict(depth=2, hidden_size=256, num_heads=2, intermediate_size=220, fullatt_block_indexes=(1,), out_hidden_size=512),
         "true80": dict(depth=2, hidden_size=1280, num_heads=16, intermediate_size=3420, fullatt_block_indexes=(1,), out_hidden_size=2048)}[name]
    t = _tiny_text()
    if name == "true80":
        t["hidden_size"], t["num_attention_heads"] = 2048, 16
    ids = dict(image_token_id=2040, video_token_id=2041, vision_start_token_id=2042, vision_end_token_id=2043)
    cfg = MR.RefConfig(vision=MR.VisionCfg(**v), text=MR.TextCfg(**t), **ids)
    geom = ModelGeometry(vision=VisionGeometry(**v), text=TextGeometry(**t), eos_token_id=2044, pad_token_id=2045, **ids)
    return cfg, geom


# image 0: 8 x 16 patches = two exact 64-token windows; image 1: 10 x 14 = ragged windows.  268 rows together.
GRIDS = [(1, 8, 16), (1, 10, 14)]


def small_pixels(cfg, seed=5):
    """bf16-representable float32 pixel rows [268, C * T * p * p] in the range of normalised images."""
    v = cfg.vision
    pd = v.in_channels * v.temporal_patch_size * v.patch_size * v.patch_size
    n = sum(h * w for _, h, w in GRIDS)
    g = torch.Generator().manual_seed(seed)
    return MR.r(torch.randn(n, pd, generator=g).clamp_(-1.8, 2.1))


def rms(x):
    return float(torch.as_tensor(x).double().pow(2).mean().sqrt())

