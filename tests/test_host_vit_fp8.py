"""CPU tests of the opt-in fp8 vision tower (sr_config.v_weight_dtype = 2): the definition's weight view, the workspace and validation rules of the
library (which size and validate without a GPU), the Python switch and the strategy's YAML key."""
import ctypes as C

import pytest
import torch

from tests import vit_fp8_ref as VR


def _cfg(geom, **kw):
    from socioreasoner_amd.engine import _sr_config
    return _sr_config(geom, 4096, 1024, 2, 256, 16, **kw)


@pytest.fixture(scope="module")
def L():
    from socioreasoner_amd import lib
    return lib.load()


def test_weight_view_quantises_exactly_the_seven_linears():
    """QuantW + mx_act for attn.qkv / attn.proj / mlp.gate_proj / mlp.up_proj / mlp.down_proj of every block and merger.mlp.0 / .2; the patch
    embedding, norm weights, every bias and the LM pass through as the tensors they are."""
    from oracle import model_ref as MR
    from oracle import weights as WG
    cfg, _ = VR.small_configs("small128")
    base = WG.LazyWeights(cfg, seed=0, fast=True)
    W = VR.VitFp8Weights(base)
    quantised = [n for n in base.specs if isinstance(W[n], MR.QuantW)]
    want = [f"visual.blocks.{i}.{s}.weight" for i in range(cfg.vision.depth) for s in ("attn.qkv", "attn.proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")]
    want += ["visual.merger.mlp.0.weight", "visual.merger.mlp.2.weight"]
    assert sorted(quantised) == sorted(want)
    assert all(W[n].mx_act for n in quantised)
    for n in ("visual.patch_embed.proj.weight", "visual.blocks.0.norm1.weight", "visual.blocks.1.attn.qkv.bias", "visual.blocks.0.mlp.down_proj.bias",
              "visual.merger.ln_q.weight", "visual.merger.mlp.0.bias", "model.layers.0.self_attn.q_proj.weight", "model.embed_tokens.weight"):
        assert W[n] is base[n], n
    # the definition: scale = amax / 448 per output channel, e4m3 elements
    w = base["visual.blocks.0.attn.proj.weight"]
    q = W["visual.blocks.0.attn.proj.weight"]
    assert torch.equal(q.scale, w.abs().amax(1) / 448.0) and q.q8.dtype == torch.float8_e4m3fn


def test_workspace_is_unchanged_with_the_switch_off(L):
    from socioreasoner_amd import lib
    from socioreasoner_amd.config import geometry_3b, geometry_tiny
    assert lib.SrConfig._fields_[-1][0] == "v_weight_dtype"          # appended: every earlier field keeps its offset
    for geom in (geometry_tiny(), geometry_3b()):
        dflt = _cfg(geom)                                            # field left at its default
        off = _cfg(geom)
        off.v_weight_dtype = 0
        n0, n1 = L.sr_workspace_bytes(C.byref(dflt)), L.sr_workspace_bytes(C.byref(off))
        assert n0 == n1 and n0 > 0
    # switched on it grows by the fp8 images, their scales and the tower's own staging buffers; the LM switch does not move that difference
    g = geometry_3b()
    on, both, lm = _cfg(g, vit_fp8="mx"), _cfg(g, vit_fp8="mx", lm_fp8="mx"), _cfg(g, lm_fp8="mx")
    grow = L.sr_workspace_bytes(C.byref(on)) - L.sr_workspace_bytes(C.byref(_cfg(g)))
    v = g.vision
    ip = (v.intermediate_size + 63) // 64 * 64
    images = v.depth * (4 * v.hidden_size ** 2 + 3 * ip * v.hidden_size) + (4 * v.hidden_size) ** 2 + v.out_hidden_size * 4 * v.hidden_size
    assert images <= grow <= images + 4096 * ip + (1 << 22)           # + scales, 4096 x 3456 staging bytes, scale blocks, alignment
    assert abs((L.sr_workspace_bytes(C.byref(both)) - L.sr_workspace_bytes(C.byref(lm))) - grow) <= 1 << 16


def test_all_six_switch_combinations_are_valid_for_a_supported_geometry(L):
    _, geom = VR.small_configs("true80")
    for lm in (False, True, "mx"):
        for vit in (False, "mx"):
            c = _cfg(geom, lm_fp8=lm, vit_fp8=vit)
            assert (c.lm_weight_dtype, c.v_weight_dtype) == ({False: 0, True: 1, "mx": 2}[lm], 2 if vit else 0)
            assert L.sr_workspace_bytes(C.byref(c)) > 0, (lm, vit, L.sr_last_error(None))


def test_unsupported_widths_are_refused_by_name(L):
    """geometry_tiny's tower is 320 wide: no multiple of the 128-wide k-tile.  The Python check and the library both say which width."""
    from socioreasoner_amd.config import check_supported, geometry_tiny
    for name in ("small128", "true80"):
        check_supported(VR.small_configs(name)[1], vit_fp8="mx")
    check_supported(geometry_tiny())                                 # fine without the mode
    with pytest.raises(ValueError, match=r"vit_fp8: vision hidden_size 320 is not a multiple"):
        check_supported(geometry_tiny(), vit_fp8="mx")
    c = _cfg(geometry_tiny(), vit_fp8="mx")
    assert L.sr_workspace_bytes(C.byref(c)) == 0
    msg = L.sr_last_error(None).decode()
    assert "v_weight_dtype 2" in msg and "hidden_size" in msg and "320" in msg, msg
    # the padded intermediate size is checked as its own width
    from socioreasoner_amd.config import ModelGeometry
    cfg, g = VR.small_configs("small128")
    g.vision.intermediate_size = 300                                 # padded to 320
    with pytest.raises(ValueError, match=r"intermediate_size padded to 64 320"):
        check_supported(g, vit_fp8="mx")
    assert L.sr_workspace_bytes(C.byref(_cfg(g, vit_fp8="mx"))) == 0 and "intermediate_size" in L.sr_last_error(None).decode()
    assert isinstance(g, ModelGeometry)


def test_value_one_is_refused_by_name(L):
    _, geom = VR.small_configs("small128")
    c = _cfg(geom)
    c.v_weight_dtype = 1
    assert L.sr_workspace_bytes(C.byref(c)) == 0
    assert "v_weight_dtype 1" in L.sr_last_error(None).decode()
    with pytest.raises(ValueError, match="vit_fp8"):
        _cfg(geom, vit_fp8=True)                                     # Engine(vit_fp8=...) takes False or "mx" only


def test_strategy_key_is_independent_of_quantization():
    from roll.distributed.strategy.mi355x_strategy import _vision_quantization
    assert _vision_quantization({}) is False
    assert _vision_quantization({"quantization": "fp8_mx"}) is False          # the LM's key keeps its meaning
    assert _vision_quantization({"vision_quantization": "fp8_mx"}) == "mx"
    assert _vision_quantization({"vision_quantization": "FP8_MX", "quantization": "fp8"}) == "mx"
    assert _vision_quantization({"vision_quantization": None}) is False
    with pytest.raises(ValueError, match="vision_quantization"):
        _vision_quantization({"vision_quantization": "fp8"})
