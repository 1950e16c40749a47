"""raster.resize_pil / sr_resize_pil_u8 (PIL's 8-bit Image.resize as two integer kernels) on the device: bit for bit against Pillow's own outputs
(tests/golden/pil_resample.npz and the installed Pillow), guard bytes round the output and the intermediate, the C ABI's refusals, a side stream,
and the two users of it (Mi355xStrategy._prepare, SegRasterStrategy.segment) with the device_resize switch on and off.

The sizes are the smallest at which the kernels can still go wrong: rows of W * C bytes that are neither dword-aligned nor a multiple of 4 long
(53 x 3 = 159), more than one 256-pixel run per row, up- and downscales, one-pass resizes, and two strong downscales -- 257 x 259 -> 28 x 28
(ksize 41 / 59), whose runs still fit the horizontal kernel's LDS stage, and 4 x 8192 -> 4 x 28 RGB, whose 24 KB run does not (the direct-read path)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_host_resample import FILTERS, N_GOLDEN, PAIRS, case_input, pair_id, pil_resize

pytestmark = pytest.mark.gpu
GPU_PAIRS = PAIRS + [((257, 259), (28, 28)), ((4, 8192), (4, 28))]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pil_resample.npz"))


@pytest.mark.parametrize("pair", GPU_PAIRS, ids=pair_id)
def test_resize_pil_equals_golden_and_installed_pil(golden, pair):
    from socioreasoner_amd import raster
    hw, HW = pair
    for kind in ("noise", "edge"):
        x3 = case_input(hw, kind, golden)
        for f, c in [(f, 3) for f in FILTERS] + [("bicubic", 1)]:
            x = x3 if c == 3 else np.ascontiguousarray(x3[:, :, 0])
            got = raster.resize_pil(torch.from_numpy(x).cuda(), HW[0], HW[1], f)
            assert got.dtype == torch.uint8 and tuple(got.shape) == HW + x.shape[2:]
            got = got.cpu().numpy()
            want = pil_resize(x, HW[0], HW[1], f)
            assert np.array_equal(got, want), (pair, kind, f, c, "installed PIL", int((got != want).sum()))
            if pair in PAIRS[:N_GOLDEN]:
                assert np.array_equal(got, golden[f"{hw[0]}x{hw[1]}_{HW[0]}x{HW[1]}_c{c}_{kind}_{f}_out"]), (pair, kind, f, c, "golden")


def test_resize_pil_batch_equals_single_calls(golden):
    from socioreasoner_amd import raster
    xs = [case_input((37, 53), "noise", golden), case_input((37, 53), "edge", golden), np.ascontiguousarray(case_input((37, 53), "noise", golden)[::-1])]
    for HW in ((28, 56), (37, 56), (28, 53), (37, 53)):          # both passes, one pass each, the copy
        got = raster.resize_pil(torch.from_numpy(np.stack(xs)).cuda(), HW[0], HW[1])
        assert tuple(got.shape) == (3,) + HW + (3,)
        for i, x in enumerate(xs):
            one = raster.resize_pil(torch.from_numpy(x).cuda(), HW[0], HW[1])
            assert torch.equal(got[i], one), (HW, i)
            assert np.array_equal(one.cpu().numpy(), pil_resize(x, HW[0], HW[1], "bicubic")), (HW, i)


def _tables(n_in, n_out, f="bicubic"):
    from socioreasoner_amd import hostops
    kk, b = hostops.pil_resample_coeffs(n_in, n_out, f)
    return torch.from_numpy(kk).cuda(), torch.from_numpy(b).cuda(), int(kk.shape[1])


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else None


@pytest.mark.parametrize("c", [3, 1])
def test_guard_bytes_round_output_and_intermediate(golden, c):
    """Source, destination and intermediate at odd byte offsets inside sentinel-filled buffers, through the C ABI: the resize is PIL's and no byte
    outside the n * H * W * C of the destination / the n * h * W * C of the intermediate changes."""
    from socioreasoner_amd import lib
    L = lib.load()
    (h, w), n = (37, 53), 2
    x = np.stack([case_input((h, w), "noise", golden), case_input((h, w), "edge", golden)])
    x = x if c == 3 else np.ascontiguousarray(x[..., 0])
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (H, W) in ((28, 56), (37, 56), (28, 53)):
        for off in (1, 2, 3, 64):
            GUARD = 256
            src = torch.full((GUARD + x.size + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
            src[off:off + x.size] = torch.from_numpy(x.reshape(-1)).cuda()
            n_dst, n_tmp = n * H * W * c, n * h * W * c
            dst = torch.full((GUARD + n_dst + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            tmp = torch.full((GUARD + n_tmp + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
            kh, kv = _tables(w, W), _tables(h, H)
            rc = L.sr_resize_pil_u8(_p(src, off), h, w, _p(dst, GUARD - off), H, W, c, n, _p(kh[0]), _p(kh[1]), kh[2], _p(kv[0]), _p(kv[1]), kv[2],
                                    _p(tmp, GUARD + off), s)
            assert rc == 0, (rc, lib.load().sr_last_error(None))
            torch.cuda.synchronize()
            d, t = dst.cpu().numpy(), tmp.cpu().numpy()
            lo = GUARD - off
            assert (d[:lo] == 0xA5).all() and (d[lo + n_dst:] == 0xA5).all(), (H, W, off, "destination guard")
            body = d[lo:lo + n_dst].reshape((n, H, W) + x.shape[3:])
            for i in range(n):
                assert np.array_equal(body[i], pil_resize(x[i], H, W, "bicubic")), (H, W, off, i)
            lo = GUARD + off
            assert (t[:lo] == 0xC3).all(), (H, W, off, "intermediate guard")
            if H != h and W != w:
                assert (t[lo + n_tmp:] == 0xC3).all(), (H, W, off, "intermediate guard")
                for i in range(n):          # the intermediate IS the horizontal pass of every source row
                    assert np.array_equal(t[lo:lo + n_tmp].reshape((n, h, W) + x.shape[3:])[i], pil_resize(x[i], h, W, "bicubic")), (H, W, off, i)
            else:
                assert (t == 0xC3).all(), (H, W, off, "a single pass does not touch the intermediate")


def test_refusals_return_minus_22_and_launch_nothing():
    from socioreasoner_amd import lib
    L = lib.load()
    h, w, H, W = 37, 53, 28, 56
    src = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    dst = torch.full((H * W * 4 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    tmp = torch.full((h * W * 4 + 64,), 0xC3, dtype=torch.uint8, device="cuda")
    kh, kv = _tables(w, W), _tables(h, H)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(sh=h, sw=w, dh=H, dw=W, c=3, n=1, th=kh, tv=kv, t=tmp):
        return L.sr_resize_pil_u8(_p(src), sh, sw, _p(dst), dh, dw, c, n, _p(th[0]), _p(th[1]), th[2], _p(tv[0]), _p(tv[1]), tv[2], _p(t), s)
    none = (None, None, 0)
    bad = {"4 channels": dict(c=4), "2 channels": dict(c=2), "0 channels": dict(c=0), "source height 0": dict(sh=0), "source width 8193": dict(sw=8193),
           "target height 8193": dict(dh=8193), "target width 0": dict(dw=0), "negative side": dict(dh=-1), "n_img 0": dict(n=0), "n_img -1": dict(n=-1),
           "no horizontal table": dict(th=none), "no horizontal bounds": dict(th=(kh[0], None, kh[2])), "no vertical table": dict(tv=none),
           "no vertical taps": dict(tv=(None, kv[1], kv[2])), "no intermediate": dict(t=None)}
    for name, kw in bad.items():
        assert call(**kw) == -22, name
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all()) and bool((tmp == 0xC3).all())
    # what is NOT refused: a pass that does not run needs neither its table nor the intermediate
    assert L.sr_resize_pil_u8(_p(src), h, w, _p(dst), h, W, 3, 1, _p(kh[0]), _p(kh[1]), kh[2], None, None, 0, None, s) == 0
    assert L.sr_resize_pil_u8(_p(src), h, w, _p(dst), H, w, 3, 1, None, None, 0, _p(kv[0]), _p(kv[1]), kv[2], None, s) == 0
    assert L.sr_resize_pil_u8(_p(src), h, w, _p(dst), h, w, 3, 1, None, None, 0, None, None, 0, None, s) == 0          # the copy
    torch.cuda.synchronize()
    assert bool((dst[:h * w * 3] == 0).all()) and bool((dst[max(h * W, H * w, h * w) * 3:] == 0xA5).all())


def test_side_stream_gives_the_same_bytes(golden):
    from socioreasoner_amd import raster
    x = torch.from_numpy(case_input((53, 37), "noise", golden)).cuda()
    want = raster.resize_pil(x, 84, 28, "lanczos")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = raster.resize_pil(x, 84, 28, "lanczos")
    side.synchronize()
    assert torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), pil_resize(x.cpu().numpy(), 84, 28, "lanczos"))


def _strategy():
    from roll.distributed.strategy.factory import create_strategy

    class W:   # minimal worker (as tests/test_gpu_pipeline.py)
        rank, world_size = 0, 1
        pipeline_config = type("P", (), {"prompt_length": 512, "response_length": 16})()
        worker_config = type("C", (), {"strategy_args": type("S", (), {"strategy_name": "mi355x", "strategy_config": {"max_batch": 2, "max_ctx": 512, "max_patches": 2048}})(),
                                       "model_args": type("M", (), {"model_name_or_path": "synthetic:tiny"})()})()
        rank_info = type("R", (), {"local_rank": 0})()
    st = create_strategy(W())
    st.initialize(None)
    return st


def test_prepare_and_generate_are_identical_with_device_resize_on_and_off():
    """A 500 x 380 image (smart_resize: 504 x 392) as a PIL image, as a CUDA uint8 tensor and, in streamed mode, on the upload stream: the pixels that
    reach the ViT are the host path's bit for bit, and so are the tokens of a greedy generate."""
    from PIL import Image
    from roll.distributed.scheduler.protocol import DataProto
    from socioreasoner_amd import synthetic
    st = _strategy()
    g = st.geom
    from roll.distributed.strategy.mi355x_strategy import DEVICE_RESIZE_DEFAULT
    assert st._device_resize() is DEVICE_RESIZE_DEFAULT          # unset in this strategy_config
    arr = case_input((500, 380), "noise")
    pil, dev = Image.fromarray(arr), torch.from_numpy(arr).cuda()
    want_px = torch.from_numpy(pil_resize(arr, 504, 392, "bicubic"))
    ids = synthetic.tile_prompt(g, 0, (1, 504 // g.vision.patch_size, 392 // g.vision.patch_size), n_pre=10, n_post=7)
    res = {}
    for on in (False, True):
        st.device_resize = on
        for name, im, side in (("pil", pil, False), ("cuda", dev, False), ("pil, upload stream", pil, True)):
            _, pos3, ims, grids = st._prepare(ids, [im], side_stream=side)
            res[on, name] = (ims[0].cpu(), grids, pos3)
            assert ims[0].is_cuda and ims[0].dtype == torch.uint8 and torch.equal(ims[0].cpu(), want_px), (on, name)
    for name in ("pil", "cuda", "pil, upload stream"):
        assert torch.equal(res[True, name][0], res[False, name][0]) and res[True, name][1] == res[False, name][1] == [(1, 36, 28)], name
        assert np.array_equal(res[True, name][2], res[False, name][2])
    P, pad = 320, g.pad_token_id
    row = np.full(P, pad, dtype=np.int64)
    row[P - len(ids):] = ids
    input_ids = torch.from_numpy(row[None])
    gc = {"max_new_tokens": 8, "temperature": 0, "top_p": 1.0, "top_k": 1, "num_beams": 1, "repetition_penalty": 1.0, "num_return_sequences": 1,
          "eos_token_id": [g.eos_token_id], "pad_token_id": pad}
    outs = {}
    for on in (False, True):
        st.device_resize = on
        for name, im in (("pil", pil), ("cuda", dev)):
            payload = np.empty(1, dtype=object)
            payload[0] = {"prompt_token_ids": ids.tolist(), "multi_modal_data": {"image": [im]}}
            outs[on, name] = st.generate(DataProto(batch={"input_ids": input_ids, "attention_mask": (input_ids != pad).long()},
                                                   non_tensor_batch={"multi_modal_data": payload}), gc)
    for k, v in outs.items():
        assert v.shape[1] > P and torch.equal(v, outs[False, "pil"]), k
    st.engine.close()


def test_segment_is_identical_with_device_resize_on_and_off():
    """SegRasterStrategy.segment over 96 x 96 source images (tiny Hiera geometry, scripted prompts): the masks with the resize on the device are
    the host path's; a second call on the same images finds every embedding cached; the host memo `_r756` is never filled with the switch on."""
    from PIL import Image
    from roll.distributed.scheduler.protocol import DataProto
    from roll.distributed.strategy.mi355x_strategy import SegRasterStrategy
    from socioreasoner_amd import sam2
    from tests.test_gpu_sam2 import _engine
    e, _ = _engine("tiny", torch.float32)
    images = np.empty(3, dtype=object)
    for i in range(3):
        images[i] = Image.fromarray(case_input((96, 96), "noise")[::(1 if i < 2 else -1)].copy() if i else case_input((96, 96), "edge"))
    prompts = np.empty(3, dtype=object)
    prompts[0] = [{"box": np.array([100, 120, 400, 380])}, {"box": np.array([300, 300, 700, 640]), "point_coords": np.array([[500, 470]]), "point_labels": np.array([1])}]
    prompts[1] = []
    prompts[2] = [{"box": np.array([40, 60, 350, 700])}]
    batch = DataProto(non_tensor_batch={"seg_image": images, "visual_prompt": prompts})

    def strategy(on):
        class W:
            worker_config = type("C", (), {"strategy_args": type("S", (), {"strategy_name": "seg_infer", "strategy_config": {"device_resize": on}})()})()
        st = SegRasterStrategy(W())
        st.model = sam2.Sam2Predictor(e)
        return st
    off, on = strategy(False), strategy(True)
    want = off.segment(batch)["mask"]
    assert len(off.__dict__.get("_r756", {})) == 2          # the host path resized (and memoised) the two live images
    got = on.segment(batch)["mask"]
    assert on.model.stats["encoded"] == 2 and on.model.stats["cache_hits"] == 0, on.model.stats
    for i in range(3):
        assert got[i].shape == (768, 768) and got[i].dtype == np.uint8 and np.array_equal(got[i], want[i]), i
    assert not want[1].any()
    print("mask pixels set:", [int(m.sum()) for m in want])
    for a, b in zip(off.model._cache.values(), on.model._cache.values()):          # the encoder saw the same pixels: its outputs are bit-identical
        assert a["orig_hw"] == b["orig_hw"] == (756, 756) and all(torch.equal(a[k], b[k]) for k in ("emb", "keys0", "f0", "f1"))
    again = on.segment(batch)["mask"]
    assert on.model.stats["encoded"] == 2 and on.model.stats["cache_hits"] == 2, on.model.stats          # cache hits only
    for i in range(3):
        assert np.array_equal(again[i], want[i]), i
    on.prefetch([images[0], images[2]])
    on.wait_prefetch()
    assert on.model.stats["encoded"] == 2 and on.model.stats["cache_hits"] == 4, on.model.stats          # the prefetch keys are segment's
    assert not on.__dict__.get("_r756")
