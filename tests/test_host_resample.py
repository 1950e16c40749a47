"""PIL's 8-bit resampling restated on the host (hostops.pil_resample_coeffs / pil_resize_ref: the definition the device kernels of
raster.resize_pil are held to): bit for bit against Pillow's own outputs, committed (tests/golden/pil_resample.npz,
tools/make_golden_resample.py) and live; the tables' invariants; the wrapper's refusals without a GPU; the C ABI's three declarations."""
import math
import os
import re

import numpy as np
import pytest
import torch

from socioreasoner_amd import hostops, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ("bicubic", "bilinear", "lanczos")
SUPPORT = {"bicubic": 2.0, "bilinear": 1.0, "lanczos": 3.0}
# (h, w) -> (H, W); the first five are in the golden file
PAIRS = [((37, 53), (28, 56)), ((53, 37), (84, 28)), ((5, 7), (28, 28)), ((64, 64), (64, 28)), ((64, 64), (28, 64)),
         ((30, 30), (448, 448)), ((500, 380), (504, 392)), ((1024, 700), (252, 168)), ((768, 768), (756, 756))]
N_GOLDEN = 5


def pair_id(p):
    return f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}"


def case_input(hw, kind, golden=None):
    """uint8 [h, w, 3]: the golden file's input where it has one, else the same seeded construction (tools/make_golden_resample.py make_input)."""
    key = f"{hw[0]}x{hw[1]}_{kind}_in"
    if golden is not None and key in golden:
        return golden[key]
    rng = np.random.default_rng(1000 * hw[0] + hw[1])
    if kind == "noise":
        return rng.integers(0, 256, hw + (3,), dtype=np.uint8)
    return (rng.integers(0, 2, hw + (3,), dtype=np.uint8) * 255).astype(np.uint8)


def pil_resize(x, H, W, filter):
    from PIL import Image
    return np.asarray(Image.fromarray(x).resize((W, H), resample={"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "lanczos": Image.LANCZOS}[filter]))


def cases():
    """(pair, filter, channels): three filters with 3 channels, bicubic also with 1."""
    return [(p, f, c) for p in PAIRS for f, c in [(f, 3) for f in FILTERS] + [("bicubic", 1)]]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pil_resample.npz"))


@pytest.mark.parametrize("pair,filter,c", cases(), ids=lambda v: pair_id(v) if isinstance(v, tuple) else str(v))
def test_pil_resize_ref_equals_golden_and_installed_pil(golden, pair, filter, c):
    (hw, HW) = pair
    for kind in ("noise", "edge"):
        x = case_input(hw, kind, golden)
        x = x if c == 3 else np.ascontiguousarray(x[:, :, 0])
        got = hostops.pil_resize_ref(x, HW[0], HW[1], filter)
        assert got.dtype == np.uint8 and got.shape == HW + x.shape[2:]
        want = pil_resize(x, HW[0], HW[1], filter)
        assert np.array_equal(got, want), (pair, filter, c, kind, "installed PIL", int((got != want).sum()))
        key = f"{hw[0]}x{hw[1]}_{HW[0]}x{HW[1]}_c{c}_{kind}_{filter}_out"
        if PAIRS.index(pair) < N_GOLDEN:
            assert np.array_equal(got, golden[key]), (pair, filter, c, kind, "golden, Pillow " + str(golden["pillow_version"]))
        else:
            assert key not in golden


def test_golden_file_is_small_and_complete(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "pil_resample.npz")) < 200 * 1000
    assert str(golden["pillow_version"])
    n = sum(1 for k in golden.files if k.endswith("_out"))
    assert n == N_GOLDEN * 2 * (len(FILTERS) + 1), n


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
@pytest.mark.parametrize("filter", FILTERS)
def test_pil_resample_coeffs_tables(pair, filter):
    """ksize and bounds as Pillow's precompute_coeffs defines them; every row sums to 2^22 within the rounding of its taps; bounds inside the input."""
    for n_in, n_out in zip(*pair):
        kk, bounds = hostops.pil_resample_coeffs(n_in, n_out, filter)
        scale = n_in / n_out
        support = SUPPORT[filter] * max(scale, 1.0)
        ksize = int(math.ceil(support)) * 2 + 1
        assert kk.dtype == np.int32 and bounds.dtype == np.int32 and kk.shape == (n_out, ksize) and bounds.shape == (n_out, 2)
        for xx in range(n_out):
            center = (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), n_in) - xmin
            assert (int(bounds[xx, 0]), int(bounds[xx, 1])) == (xmin, xmax), xx
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= ksize).all() and (bounds.sum(1) <= n_in).all()
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()       # what the horizontal kernel's run span relies on
        assert (np.abs(kk.astype(np.int64).sum(1) - (1 << 22)) <= ksize).all()
        for xx in range(n_out):
            assert not kk[xx, bounds[xx, 1]:].any()                                             # unused taps are 0
        assert np.abs(kk.astype(np.int64)).sum(1).max() * 255 + (1 << 21) < 2 ** 31              # the int32 accumulator of both passes


def test_pil_resize_ref_refuses_by_name():
    with pytest.raises(ValueError, match="filter"):
        hostops.pil_resample_coeffs(8, 4, "nearest")
    with pytest.raises(ValueError, match="arr_u8_hwc.*4 channels"):
        hostops.pil_resize_ref(np.zeros((4, 4, 4), np.uint8), 2, 2)
    with pytest.raises(ValueError, match="arr_u8_hwc"):
        hostops.pil_resize_ref(np.zeros((4, 4, 3), np.float32), 2, 2)


def test_resize_pil_refuses_before_the_library_is_loaded(monkeypatch):
    from socioreasoner_amd import raster

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(lib, "load", no_load)
    with pytest.raises(ValueError, match="src.*4 channels"):
        raster.resize_pil(torch.zeros(8, 8, 4, dtype=torch.uint8), 4, 4)
    with pytest.raises(ValueError, match="filter"):
        raster.resize_pil(torch.zeros(8, 8, 3, dtype=torch.uint8), 4, 4, filter="hamming")
    with pytest.raises(ValueError, match="src.*uint8"):
        raster.resize_pil(torch.zeros(8, 8, 3, dtype=torch.float32), 4, 4)
    with pytest.raises(ValueError, match="8192"):
        raster.resize_pil(torch.zeros(8, 8, 3, dtype=torch.uint8), 4, 8193)


def test_sr_resize_pil_u8_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "socior.h")).read()
    m = re.search(r"\bint\s+sr_resize_pil_u8\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/socior.h does not declare sr_resize_pil_u8"
    params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    assert len(params) == 16, params
    vs = open(os.path.join(ROOT, "socioreasoner_amd", "csrc", "exports.map")).read()
    globs = re.findall(r"global:\s*([^;]+);", vs)
    import fnmatch
    assert any(fnmatch.fnmatchcase("sr_resize_pil_u8", g.strip()) for g in globs), vs
    res, args = lib.SIGNATURES["sr_resize_pil_u8"]
    import ctypes as C
    assert res is C.c_int and len(args) == 16
    assert [a for a in args if a is C.c_int] == [C.c_int] * 8 and [a for a in args if a is C.c_void_p] == [C.c_void_p] * 8


def test_device_resize_switch_is_read_from_the_strategy_config():
    from roll.distributed.strategy.mi355x_strategy import DEVICE_RESIZE_DEFAULT, Mi355xStrategy, SegRasterStrategy

    def worker(sc):
        class W:
            worker_config = type("C", (), {"strategy_args": type("S", (), {"strategy_name": "x", "strategy_config": sc})()})()
        return W()
    for cls in (Mi355xStrategy, SegRasterStrategy):
        assert cls(worker({}))._device_resize() is DEVICE_RESIZE_DEFAULT and cls(worker(None))._device_resize() is DEVICE_RESIZE_DEFAULT
        assert cls(worker({"device_resize": False}))._device_resize() is False
        assert cls(worker({"device_resize": True}))._device_resize() is True

    class Foreign:          # a predictor without resize_to (the reference's SAM2ImagePredictor shape): the host path
        def segment_batch(self, images, prompts):
            return []
    st = SegRasterStrategy(worker({"device_resize": True}))
    st.model = Foreign()
    assert st._resize_on_device([]) is False
