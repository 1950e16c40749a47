"""Host references of the SAM2 pass kernels (socioreasoner_amd/csrc/sam.hip: k_sam_preprocess, k_im2col, k_layernorm, k_layernorm_v<32,1 |
64,1 | 64,2 | 64,3>, k_maxpool_win, k_ew, k_transpose, k_transpose_v, k_upsample2x_add, k_pixel_shuffle_add, k_mask_resize_or; elementwise.hip:
k_gather_rows), plain torch / numpy on the CPU in float64.  Not a test module: tests/test_host_sam2_ops_ref.py pins it against independent
torch forms, tests/test_gpu_sam2_ops.py holds the kernels to it through the sr_op_* entry points.

A case is what the C ABI takes: flat buffers (the pointer an entry point gets is ``buffer + off[name]`` elements) and the integer arguments
in ``Built.p``.  Three things are computed from it:

  * ``reference(b)``   : per output buffer ``(want, written)`` -- float64 values over the WHOLE buffer (offset, pad columns, the rows past the
    end and the guard region included) and the boolean map of the elements the op defines.  Written from the operation's definition
    (F.layer_norm, F.unfold, F.max_pool2d on the un-windowed map, F.pixel_shuffle, F.interpolate, indexing), not from the kernels' index
    arithmetic.
  * ``restate32(b)``   : the same formula in numpy float32 with the kernel's order of operations, for the ops that round (preprocess,
    layernorm, ew modes 3 / 4, mask resize).  It is never compared with a kernel: it only measures how far float32 evaluation sits from
    float64 on the case, which sizes the bound the kernel gets (``bounds``).
  * ``check_preconditions(b)`` : the executable form of what the kernels assume and do not check (include/socior.h), asserted before every
    launch of the GPU test and over the whole table on the CPU.

The second half is the case table and the generator of its inputs.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sam2_ref as SR
from tests.attention_ref import _GARBAGE, _bits
from tests.util import bf16_compare

SENT_BF16 = 0x7fc1                    # quiet-NaN patterns no kernel produces from finite inputs
SENT_F32 = 0x7fc00a51
GUARD_U8 = 0xAA
GUARD_ROWS = 2                        # rows after the last one of every matrix: guard region of an output, "rows past the end" of an input
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EXACT_OPS = ("im2col", "maxpool_win", "transpose", "gather_rows", "upsample2x_add", "pixel_shuffle_add")
F32_ENTRY = ("sam_preprocess", "im2col", "layernorm", "maxpool_win", "ew", "upsample2x_add", "pixel_shuffle_add")


# ================================================================================================ storage and rounding
def tdtype(storage):
    return torch.bfloat16 if storage == "bf16" else torch.float32


def round_bf16_bits(x64: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16 bit patterns (int16), ONE round-to-nearest-even (a cast through float32 would round twice on a tie)"""
    x = x64.detach().double().numpy()
    f = x.astype(np.float32)
    bits = f.view(np.uint32).astype(np.uint64)
    low, up = bits & 0xffff, bits >> 16
    tie = low == 0x8000
    resid = np.abs(x) - np.abs(f.astype(np.float64))
    rnd = (low > 0x8000) | (tie & ((up & 1) == 1))
    rnd = np.where(tie & (resid > 0), True, np.where(tie & (resid < 0), False, rnd))
    return torch.from_numpy((up + rnd).astype(np.uint16).view(np.int16).copy()).view(x64.shape)


def round_storage_bits(x64, storage):
    """float64 -> the storage type's bit patterns, rounded once (int16 for bf16, int32 for float32)"""
    if storage == "bf16":
        return round_bf16_bits(x64)
    return x64.to(torch.float32).view(torch.int32)


def bits_of(t: torch.Tensor) -> torch.Tensor:
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def values_of(bits: torch.Tensor, kind) -> torch.Tensor:
    if kind == "u8":
        return bits.double()
    return bits.view(tdtype(kind)).double()


def sentinel(n, kind):
    if kind == "bf16":
        return torch.full((n,), SENT_BF16, dtype=torch.int16)
    if kind == "f32":
        return torch.full((n,), SENT_F32, dtype=torch.int32)
    return torch.full((n,), GUARD_U8, dtype=torch.uint8)


def _garbage(n, storage):
    if storage == "bf16":
        return _bits(_GARBAGE, n)
    pat = np.array([np.nan, np.inf, -np.inf, 3.4e38, -3.4e38], dtype=np.float32)
    return torch.from_numpy(np.tile(pat, n // len(pat) + 1)[:n].copy())


# ================================================================================================ cases
@dataclass
class Case:
    name: str
    op: str
    storage: str                  # "bf16" | "f32": the element type of the matrices (mask_resize_or: "f32", gather_rows: what the rows hold)
    kernel: str                   # the kernel the launch must reach (checked against the launcher's dispatch rule by check_preconditions)
    p: dict
    seed_name: str = ""           # cases that share it get the same logical input (the vector / scalar twins)

    @property
    def seed(self):
        return zlib.crc32((self.seed_name or self.name).encode()) & 0x7fffffff


@dataclass
class Out:
    init: torch.Tensor            # bit patterns the buffer holds before the launch (sentinel, or the input of an in-place case)
    kind: str                     # "bf16" | "f32" | "u8"
    alias: str = ""               # in place: the input buffer this output IS


@dataclass
class Built:
    case: Case
    p: dict
    bufs: dict                    # name -> flat host tensor
    off: dict = field(default_factory=dict)       # name -> element offset of the pointer the entry point gets
    outs: dict = field(default_factory=dict)      # name -> Out

    def _t(self, name):
        return self.outs[name].init if name in self.outs else self.bufs[name]

    def numel(self, name):
        return self._t(name).numel()

    def avail(self, name):
        return self.numel(name) - self.off.get(name, 0)

    def itemsize(self, name):
        return self._t(name).element_size()

    def aligned16(self, name):
        return (self.off.get(name, 0) * self.itemsize(name)) % 16 == 0        # device allocations themselves are 256-byte aligned


def _matrix(b: Built, name, vals: torch.Tensor, ld, garbage, off=0):
    """flat buffer [off + (rows + GUARD_ROWS) * ld] holding ``vals`` [rows, C] in its live columns; pad columns, the rows past the end and
    the offset prefix hold zeros, or NaN / inf patterns with ``garbage``"""
    rows, C = vals.shape
    st = b.case.storage
    n = off + (rows + GUARD_ROWS) * ld
    buf = _garbage(n, st).clone() if garbage else torch.zeros(n, dtype=tdtype(st))
    buf[off: off + (rows + GUARD_ROWS) * ld].view(rows + GUARD_ROWS, ld)[:rows, :C] = vals.to(tdtype(st))
    b.bufs[name] = buf
    if off:
        b.off[name] = off
    return buf


def _out(b: Built, name, rows, ld, off=0, kind=None):
    kind = kind or b.case.storage
    b.outs[name] = Out(sentinel(off + (rows + GUARD_ROWS) * ld, kind), kind)
    if off:
        b.off[name] = off


def _inplace(b: Built, name, alias):
    b.outs[name] = Out(bits_of(b.bufs[alias]).clone(), b.case.storage, alias)
    if alias in b.off:
        b.off[name] = b.off[alias]


def view(b: Built, name, rows, ld):
    """[rows, ld] view of an input buffer, from the pointer the entry point gets"""
    o = b.off.get(name, 0)
    return b.bufs[name][o: o + rows * ld].view(rows, ld)


def T_of(p):
    return (p["S"] + 2 * p["pad"] - p["k"]) // p["stride"] + 1


def _blob(m):
    y, x = torch.meshgrid(torch.arange(m, dtype=torch.float64), torch.arange(m, dtype=torch.float64), indexing="ij")
    return (6.0 * torch.exp(-((y - 0.4 * m) ** 2 + (x - 0.55 * m) ** 2) / (2 * (0.22 * m) ** 2)) - 2.0).float()


def build(case: Case, garbage=False) -> Built:
    """The launch of a case.  ``garbage``: NaN / inf patterns instead of zeros in every input element the op must not use (pad columns,
    rows past the end, the prefix of an offset pointer); the live elements are the same."""
    g = torch.Generator().manual_seed(case.seed)
    p = dict(case.p)
    st = case.storage
    b = Built(case, p, {})
    rn = lambda *s: torch.randn(*s, generator=g)
    op = case.op
    if op == "layernorm":
        rows, C, ldx, ldo = p["rows"], p["C"], p["ldx"], p["ldo"]
        kind = p.get("input", "normal")
        if kind == "constant":
            x = (rn(rows, 1) * 2.0).to(tdtype(st)).float().expand(rows, C).clone()
        elif kind == "mean100":
            x = 100.0 + 0.1 * rn(rows, C)
        else:
            x = rn(rows, C) * (0.5 + 2.0 * torch.rand(rows, 1, generator=g)) + rn(rows, 1)
        w, bias = 1.0 + 0.3 * rn(1, C), 0.5 * rn(1, C)
        p["eps"] = float(np.float32(p.get("eps", 1e-6)))
        _matrix(b, "x", x, ldx, garbage, off=p.get("x_off", 0))
        _matrix(b, "w", w, C + 8, garbage)
        _matrix(b, "b", bias, C + 8, garbage)
        if p.get("inplace"):
            assert ldx == ldo
            _inplace(b, "out", "x")
        else:
            _out(b, "out", rows, ldo)
    elif op == "transpose":
        rows, cols = p["rows"], p["cols"]
        _matrix(b, "in", rn(rows, cols), p["ld_in"], garbage)
        _out(b, "out", cols, p["ld_out"], off=p.get("out_off", 0))
    elif op == "maxpool_win":
        C, n_win, ws = p["C"], p["n_win"], p["ws"]
        x = rn(n_win * ws * ws, C)
        if p.get("negative"):
            x = -x.abs() - 0.25
        _matrix(b, "in", x, p["ld_in"], garbage)
        _out(b, "out", n_win * (ws // 2) ** 2, p["ld_out"])
    elif op == "ew":
        rows, C, mode = p["rows"], p["C"], p["mode"]
        wide = mode in (3, 4)
        a = (torch.rand(rows, C, generator=g) * 16.0 - 8.0) if wide else rn(rows, C) * 3.0
        bb = rn(1 if mode == 1 else rows, C) * 2.0
        _matrix(b, "a", a, p["lda"], garbage)
        _matrix(b, "b", bb, p["ldb"], garbage)
        if p.get("inplace"):
            assert p["lda"] == p["ldo"]
            _inplace(b, "out", "a")
        else:
            _out(b, "out", rows, p["ldo"])
    elif op == "upsample2x_add":
        H2, C, ld = p["H2"], p["C"], p["ld"]
        _matrix(b, "lat", rn(H2 * H2, C), ld, garbage)
        _matrix(b, "top", rn((H2 // 2) ** 2, C), ld, garbage)
        _out(b, "out", H2 * H2, ld)
    elif op == "pixel_shuffle_add":
        W, Co = p["W"], p["Co"]
        _matrix(b, "g", rn(W * W, 4 * Co), p["ldg"], garbage)
        _matrix(b, "feat", rn(4 * W * W, Co), p["ldf"], garbage)
        _out(b, "out", 4 * W * W, p["ldo"])
    elif op == "im2col":
        S, T = p["S"], T_of(p)
        _matrix(b, "chw", rn(1, 3 * S * S), 3 * S * S, garbage)
        if p.get("rowmap"):
            b.bufs["rowmap"] = torch.randperm(T * T, generator=g).to(torch.int32)
        _out(b, "out", T * T, p["ld"])
    elif op == "sam_preprocess":
        h, w, S = p["h"], p["w"], p["S"]
        img = torch.randint(0, 256, (h * w * 3,), generator=g, dtype=torch.int32).to(torch.uint8)
        b.bufs["img"] = torch.cat([img, torch.full((64,), 0xff if garbage else 0, dtype=torch.uint8)])
        _out(b, "out", 1, 3 * S * S)
    elif op == "mask_resize_or":
        m, h, w, n, col0, ld = p["m"], p["h"], p["w"], p["n"], p["col0"], p["ld"]
        kind = p.get("input", "random")
        if kind == "zero":
            maps = torch.zeros(m * m, n)
        elif kind == "blob":
            maps = torch.stack([_blob(m).flatten() * (1.0 + 0.5 * i) for i in range(n)], dim=1)
        else:
            maps = rn(m * m, n) * 5.0
        low = _garbage((m * m + GUARD_ROWS) * ld, "f32").clone() if garbage else torch.zeros((m * m + GUARD_ROWS) * ld)
        low.view(-1, ld)[: m * m, col0: col0 + n] = maps
        b.bufs["low"] = low
        score = _garbage(ld, "f32").clone() if garbage else torch.zeros(ld)
        sc = torch.rand(n, generator=g)
        if p.get("tie"):
            sc[:] = 0.5                    # every score equal: the first wins
            if n > 2:
                sc[0] = 0.25               # ... and the first of the two that tie for the maximum, when the maximum is not column 0
        score[col0: col0 + n] = sc
        b.bufs["score"] = score
        acc = sentinel(h * w + 64, "u8")
        acc[: h * w] = (torch.rand(h * w, generator=g) < 0.05).to(torch.uint8)        # bits an earlier object set: they stay
        b.outs["acc"] = Out(acc, "u8")
        b.outs["logits"] = Out(sentinel(n * h * w + 64, "f32"), "f32")
    elif op == "gather_rows":
        n, H, n_in = p["n"], p["H"], p["n_in"]
        Hs = H // 2 if st == "f32" else H              # the float32 use: a float32 row is 2 * Hs bf16 elements
        _matrix(b, "in", rn(n_in, Hs), Hs, garbage)
        idx = torch.randint(0, n_in, (n,), generator=g, dtype=torch.int32)
        if n > 2:
            idx[n - 1] = idx[1]            # a duplicate
            idx[0] = n_in - 1              # the last row
        b.bufs["rows"] = idx
        _out(b, "out", n, Hs)
    else:
        raise KeyError(op)
    return b


# ================================================================================================ float64 references
def _place(b, name, rows, ld, vals2d, written2d):
    n = b.numel(name)
    o = b.off.get(name, 0)
    want, written = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.bool)
    want[o: o + rows * ld].view(rows, ld)[:] = vals2d
    written[o: o + rows * ld].view(rows, ld)[:] = written2d
    return want, written


def _cols(rows, ld, C):
    w = torch.zeros(rows, ld, dtype=torch.bool)
    w[:, :C] = True
    return w


def gelu64(x):
    return F.gelu(x.double())


def interp64(maps, size):
    """[n, sh, sw] float64 -> [n, h, w]: bilinear, align_corners False (F.interpolate, what HF / torchvision run)"""
    return F.interpolate(maps.double()[None], size=size, mode="bilinear", align_corners=False)[0]


def preprocess64(img_u8, S):
    """oracle.sam2_ref.preprocess with float64 in place of float32: [3, S, S]"""
    x = img_u8.permute(2, 0, 1).double() / 255.0
    x = interp64(x, (S, S))
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float64).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float64).view(3, 1, 1)
    return (x - mean) / std


def best_of(b):
    p = b.p
    return int(np.argmax(b.bufs["score"][p["col0"]: p["col0"] + p["n"]].numpy()))           # numpy: the FIRST maximum


def mask_logits64(b):
    p = b.p
    m, n, col0 = p["m"], p["n"], p["col0"]
    maps = b.bufs["low"].view(-1, p["ld"])[: m * m, col0: col0 + n].t().reshape(n, m, m)
    return interp64(maps, (p["h"], p["w"]))


def reference(b: Built) -> dict:
    p, op = b.p, b.case.op
    if op == "layernorm":
        rows, C, ldo = p["rows"], p["C"], p["ldo"]
        x = view(b, "x", rows, p["ldx"])[:, :C].double()
        y = F.layer_norm(x, (C,), b.bufs["w"][:C].double(), b.bufs["b"][:C].double(), p["eps"])
        out = torch.zeros(rows, ldo, dtype=torch.float64)
        out[:, :C] = y
        return {"out": _place(b, "out", rows, ldo, out, _cols(rows, ldo, ldo))}
    if op == "transpose":
        rows, cols, ldo = p["rows"], p["cols"], p["ld_out"]
        out = torch.zeros(cols, ldo, dtype=torch.float64)
        out[:, :rows] = view(b, "in", rows, p["ld_in"])[:, :cols].double().t()
        return {"out": _place(b, "out", cols, ldo, out, _cols(cols, ldo, rows))}
    if op == "maxpool_win":
        C, n_win, ws, ldo = p["C"], p["n_win"], p["ws"], p["ld_out"]
        x = view(b, "in", n_win * ws * ws, p["ld_in"])[:, :C].double().reshape(n_win, ws * ws, C)
        full = SR._unwindows(x, ws, ws, n_win * ws)                                   # the windows side by side: [ws, n_win * ws, C]
        pooled = SR._pool(full).contiguous()                                          # F.max_pool2d(2, 2)
        y = SR._windows(pooled, ws // 2).reshape(-1, C).double()
        rows = n_win * (ws // 2) ** 2
        out = torch.zeros(rows, ldo, dtype=torch.float64)
        out[:, :C] = y
        return {"out": _place(b, "out", rows, ldo, out, _cols(rows, ldo, C))}
    if op == "ew":
        rows, C, mode, ldo = p["rows"], p["C"], p["mode"], p["ldo"]
        a = view(b, "a", rows, p["lda"])[:, :C].double()
        bb = view(b, "b", 1 if mode == 1 else rows, p["ldb"])[:, :C].double()
        y = (a + bb, a + bb, torch.relu(a), gelu64(a), F.silu(a) * bb)[mode]
        out = torch.zeros(rows, ldo, dtype=torch.float64)
        out[:, :C] = y
        return {"out": _place(b, "out", rows, ldo, out, _cols(rows, ldo, C))}
    if op == "upsample2x_add":
        H2, C, ld = p["H2"], p["C"], p["ld"]
        lat = view(b, "lat", H2 * H2, ld)[:, :C].double().reshape(H2, H2, C)
        top = view(b, "top", (H2 // 2) ** 2, ld)[:, :C].double().reshape(H2 // 2, H2 // 2, C)
        y = lat + top.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)
        out = torch.zeros(H2 * H2, ld, dtype=torch.float64)
        out[:, :C] = y.reshape(H2 * H2, C)
        return {"out": _place(b, "out", H2 * H2, ld, out, _cols(H2 * H2, ld, C))}
    if op == "pixel_shuffle_add":
        W, Co, ldo = p["W"], p["Co"], p["ldo"]
        gm = view(b, "g", W * W, p["ldg"])[:, : 4 * Co].double().reshape(W, W, 4 * Co).permute(2, 0, 1)      # [Co * 4, W, W]
        y = F.pixel_shuffle(gm[None], 2)[0].permute(1, 2, 0).reshape(4 * W * W, Co)
        y = y + view(b, "feat", 4 * W * W, p["ldf"])[:, :Co].double()
        out = torch.zeros(4 * W * W, ldo, dtype=torch.float64)
        out[:, :Co] = y
        return {"out": _place(b, "out", 4 * W * W, ldo, out, _cols(4 * W * W, ldo, Co))}
    if op == "im2col":
        S, k, ld, T = p["S"], p["k"], p["ld"], T_of(p)
        chw = b.bufs["chw"][: 3 * S * S].double().reshape(1, 3, S, S)
        u = F.unfold(chw, k, padding=p["pad"], stride=p["stride"])[0].t()                 # [(ty, tx)][c * k * k + ky * k + kx]
        out = torch.zeros(T * T, ld, dtype=torch.float64)
        dst = b.bufs["rowmap"].long() if "rowmap" in b.bufs else torch.arange(T * T)
        out[dst, : 3 * k * k] = u
        return {"out": _place(b, "out", T * T, ld, out, _cols(T * T, ld, ld))}
    if op == "sam_preprocess":
        h, w, S = p["h"], p["w"], p["S"]
        y = preprocess64(b.bufs["img"][: h * w * 3].reshape(h, w, 3), S).reshape(1, 3 * S * S)
        return {"out": _place(b, "out", 1, 3 * S * S, y, _cols(1, 3 * S * S, 3 * S * S))}
    if op == "mask_resize_or":
        h, w, n = p["h"], p["w"], p["n"]
        up = mask_logits64(b)
        init = b.outs["acc"].init
        acc, wa = init.double().clone(), torch.zeros(init.numel(), dtype=torch.bool)
        acc[: h * w] = ((init[: h * w] != 0) | (up[best_of(b)].flatten() > 0)).double()
        wa[: h * w] = True
        lg, wl = torch.zeros(b.outs["logits"].init.numel(), dtype=torch.float64), torch.zeros(b.outs["logits"].init.numel(), dtype=torch.bool)
        lg[: n * h * w] = up.flatten()
        wl[: n * h * w] = True
        return {"acc": (acc, wa), "logits": (lg, wl)}
    if op == "gather_rows":
        n, Hs = p["n"], b.bufs["in"].numel() // (p["n_in"] + GUARD_ROWS)
        y = view(b, "in", p["n_in"], Hs)[b.bufs["rows"].long()].double()
        return {"out": _place(b, "out", n, Hs, y, _cols(n, Hs, Hs))}
    raise KeyError(op)


# ================================================================================================ float32 restatements
f32 = np.float32


def _lanes_sum(v, lane_of, n_lanes, offsets):
    """float32 row sums in a kernel's order: each lane adds its channels in ascending order, then the lanes are combined by the xor
    butterfly with the given offsets (every lane ends with the same total)"""
    rows, C = v.shape
    part = np.zeros((rows, n_lanes), dtype=f32)
    for c in range(C):
        part[:, lane_of[c]] = part[:, lane_of[c]] + v[:, c]
    idx = np.arange(n_lanes)
    for o in offsets:
        part = part + part[:, idx ^ o]
    return part[:, 0]


def _ln_layout(kernel, C):
    c = np.arange(C)
    if kernel.startswith("k_layernorm_v"):
        LP = 32 if "<32" in kernel else 64
        return (c // 8) % LP, LP, [1 << i for i in range(LP.bit_length() - 1)]
    return c % 64, 64, [32, 16, 8, 4, 2, 1]


def bilinear(src, h_out, w_out, ft=f32):
    """k_sam_preprocess / k_mask_resize_or's resize of maps [n, sh, sw], operation by operation in the float type ``ft``"""
    n, sh, sw = src.shape
    src = src.astype(ft)
    y, x = np.arange(h_out).astype(ft), np.arange(w_out).astype(ft)
    sy = np.maximum((y + ft(0.5)) * (ft(sh) / ft(h_out)) - ft(0.5), ft(0))
    sx = np.maximum((x + ft(0.5)) * (ft(sw) / ft(w_out)) - ft(0.5), ft(0))
    y0, x0 = np.minimum(sy.astype(np.int32), sh - 1), np.minimum(sx.astype(np.int32), sw - 1)
    y1, x1 = np.minimum(y0 + 1, sh - 1), np.minimum(x0 + 1, sw - 1)
    fy, fx = (sy - y0.astype(ft))[None, :, None], (sx - x0.astype(ft))[None, None, :]
    p00, p01 = src[:, y0][:, :, x0], src[:, y0][:, :, x1]
    p10, p11 = src[:, y1][:, :, x0], src[:, y1][:, :, x1]
    top = p00 * (ft(1) - fx) + p01 * fx
    bot = p10 * (ft(1) - fx) + p11 * fx
    return (top * (ft(1) - fy) + bot * fy).astype(ft)


def restate32(b: Built) -> dict:
    """name -> float32 values over the whole output buffer (0 where nothing is defined), for the ops that are not exact"""
    p, op = b.p, b.case.op
    ref = reference(b)
    if op == "layernorm":
        rows, C, ldo = p["rows"], p["C"], p["ldo"]
        v = view(b, "x", rows, p["ldx"])[:, :C].float().numpy()
        w, bias = b.bufs["w"][:C].float().numpy(), b.bufs["b"][:C].float().numpy()
        lane_of, nl, offs = _ln_layout(b.case.kernel, C)
        mean = (_lanes_sum(v, lane_of, nl, offs) / f32(C))[:, None]
        d = v - mean
        q = _lanes_sum(d * d, lane_of, nl, offs) / f32(C) + f32(p["eps"])
        rstd = (f32(1) / np.sqrt(q, dtype=f32))[:, None]
        y = d * rstd * w + bias
        out = np.zeros((rows, ldo), dtype=f32)
        out[:, :C] = y
        return {"out": _place(b, "out", rows, ldo, torch.from_numpy(out).double(), _cols(rows, ldo, ldo))[0].float()}
    if op == "ew" and p["mode"] in (3, 4):
        rows, C, ldo = p["rows"], p["C"], p["ldo"]
        a = view(b, "a", rows, p["lda"])[:, :C].float()
        if p["mode"] == 3:
            an = a.numpy()
            y = an * f32(0.5) * (f32(1) + torch.erf(torch.from_numpy(an * f32(0.70710678118654752440))).numpy())
        else:
            an, bn = a.numpy(), view(b, "b", rows, p["ldb"])[:, :C].float().numpy()
            y = an * (f32(1) / (f32(1) + np.exp(-an, dtype=f32))) * bn
        out = np.zeros((rows, ldo), dtype=f32)
        out[:, :C] = y
        return {"out": _place(b, "out", rows, ldo, torch.from_numpy(out).double(), _cols(rows, ldo, C))[0].float()}
    if op == "sam_preprocess":
        h, w, S = p["h"], p["w"], p["S"]
        img = b.bufs["img"][: h * w * 3].reshape(h, w, 3).permute(2, 0, 1).numpy().astype(f32) / f32(255.0)
        r = bilinear(img, S, S)
        mean, std = np.array(IMAGENET_MEAN, dtype=f32)[:, None, None], np.array(IMAGENET_STD, dtype=f32)[:, None, None]
        y = ((r - mean) / std).astype(f32).reshape(1, -1)
        return {"out": _place(b, "out", 1, 3 * S * S, torch.from_numpy(y).double(), True)[0].float()}
    if op == "mask_resize_or":
        m, n, col0, h, w = p["m"], p["n"], p["col0"], p["h"], p["w"]
        maps = b.bufs["low"].view(-1, p["ld"])[: m * m, col0: col0 + n].t().reshape(n, m, m).numpy()
        lg = torch.zeros_like(ref["logits"][0], dtype=torch.float32)
        lg[: n * h * w] = torch.from_numpy(bilinear(np.ascontiguousarray(maps), h, w)).flatten()
        return {"logits": lg}
    return {}


# ================================================================================================ bounds
def f32_ulp(x):
    return 2.0 ** (np.floor(np.log2(x)) - 23) if x > 0 else 0.0


def is_exact(case: Case):
    return case.op in EXACT_OPS or (case.op == "ew" and case.p["mode"] in (0, 1, 2))


def ew_floor_mask(want):
    """ew modes 3 / 4: the differing share is counted over |want| >= rms * 2^-8 only (below it float32's 1 + erf cancellation decides the
    last bit; those elements are judged by max_ulp alone)"""
    return want.abs() >= want.pow(2).mean().sqrt() * 2.0 ** -8


def measure(b: Built, name, got64, want64, written):
    """distance of float32-evaluated values ``got64`` (the restatement on the CPU, the kernel on the GPU) to the float64 reference over the
    elements the op defines.  bf16 storage: both rounded once to bf16, (max ulp, differing share, max abs); float32: max abs error."""
    c = b.case
    g, w = got64[written], want64[written]
    if b.outs[name].kind == "bf16":
        wb = round_bf16_bits(w).view(torch.bfloat16).double()
        mu, share, mad = bf16_compare(g, wb)
        if c.op == "ew":
            big = ew_floor_mask(wb)
            share = float((g[big] != wb[big]).double().mean()) if bool(big.any()) else 0.0
        return {"max_ulp": mu, "share": share, "max_abs": mad}
    return {"max_abs": float((g - w).abs().max())}


def bounds(b: Built, name="out") -> dict:
    """What the GPU test allows the kernel on this case, from the float32 restatement's own distance to float64 (measured here, on the
    CPU): bf16 storage 1 ulp on 4 x its differing share + 1e-3; float32 storage 4 x its max abs error, at least 2 float32 ulps of the
    reference's rms."""
    want, written = reference(b)[name]
    r32 = restate32(b)[name].double()
    if b.outs[name].kind == "bf16":
        r32 = round_bf16_bits(r32).view(torch.bfloat16).double()
    own = measure(b, name, r32, want, written)
    rms = float(want[written].pow(2).mean().sqrt())
    if b.outs[name].kind == "bf16":
        return {"own": own, "max_ulp": 1.0, "frac": 4.0 * own["share"] + 1e-3, "rms": rms}
    return {"own": own, "max_abs": max(4.0 * own["max_abs"], 2.0 * f32_ulp(rms)), "rms": rms}


def pad_mask(b: Built):
    """the pad columns an op defines as zero (layernorm [C, ldo), im2col [3 k k, ld)): bit-exact zeros whatever the storage"""
    p, op = b.p, b.case.op
    if op == "layernorm":
        rows, ld, C = p["rows"], p["ldo"], p["C"]
    elif op == "im2col":
        rows, ld, C = T_of(p) ** 2, p["ld"], 3 * p["k"] ** 2
    else:
        return None
    return _place(b, "out", rows, ld, 0.0, ~_cols(rows, ld, C))[1]


def mask_exempt(b: Built, bound):
    """pixels whose float64 logit of the best map lies within ``bound`` of the threshold: float32 may land on the other side"""
    p = b.p
    v = mask_logits64(b)[best_of(b)].flatten()
    return v.abs() <= bound


# ================================================================================================ the kernels' preconditions
def dispatch(b: Built) -> str:
    """the launcher's choice of kernel (sam.hip launch_layernorm / launch_transpose), from the same quantities"""
    p, c = b.p, b.case
    if c.op == "layernorm":
        if c.storage == "f32":
            return "k_layernorm<float>"
        C, ldx, ldo = p["C"], p["ldx"], p["ldo"]
        if C % 8 == 0 and ldx % 8 == 0 and ldo % 8 == 0 and all(b.aligned16(n) for n in ("x", "out", "w", "b")):
            span = max(C, ldo)
            return "k_layernorm_v<32,1>" if span <= 256 else "k_layernorm_v<64,1>" if span <= 512 else "k_layernorm_v<64,2>" if span <= 1024 else "k_layernorm_v<64,3>"
        return "k_layernorm<bf16_t>"
    if c.op == "transpose":
        vec = p["cols"] % 8 == 0 and p["ld_in"] % 8 == 0 and p["ld_out"] % 8 == 0 and b.aligned16("in") and b.aligned16("out")
        return "k_transpose_v" if vec else "k_transpose"
    return c.kernel


def check_preconditions(b: Built):
    """Every launch the GPU test makes stays inside its buffers and satisfies what the kernels assume without checking (include/socior.h,
    the SAM2 pass entry points): asserted on the host before anything is launched."""
    p, c, op = b.p, b.case, b.case.op
    ext = lambda rows, ld, C: (rows - 1) * ld + C              # elements from the pointer to the end of the last live row
    for name in list(b.bufs) + list(b.outs):
        assert b.off.get(name, 0) >= 0 and b.avail(name) > 0, name
    assert dispatch(b) == c.kernel, (c.name, dispatch(b), c.kernel)
    if op == "layernorm":
        rows, C, ldx, ldo = p["rows"], p["C"], p["ldx"], p["ldo"]
        assert rows >= 1 and 1 <= C <= 1152 and C <= ldo <= 1152 and ldx >= C
        assert ext(rows, ldx, C) <= b.avail("x") and ext(rows, ldo, ldo) <= b.avail("out")
        assert C <= b.avail("w") and C <= b.avail("b")
        if c.storage == "f32":
            assert ldx % 4 == 0 and ldo % 4 == 0
        if b.outs["out"].alias:
            assert ldx == ldo and b.off.get("x", 0) == b.off.get("out", 0)
    elif op == "transpose":
        rows, cols, ld_in, ld_out = p["rows"], p["cols"], p["ld_in"], p["ld_out"]
        assert rows >= 1 and cols >= 1 and ld_in >= cols and ld_out >= rows
        assert ext(rows, ld_in, cols) <= b.avail("in") and ext(cols, ld_out, rows) <= b.avail("out")
    elif op == "maxpool_win":
        C, n_win, ws = p["C"], p["n_win"], p["ws"]
        assert ws % 2 == 0 and ws >= 2 and n_win >= 1 and C >= 1 and p["ld_in"] >= C and p["ld_out"] >= C
        assert ext(n_win * ws * ws, p["ld_in"], C) <= b.avail("in") and ext(n_win * (ws // 2) ** 2, p["ld_out"], C) <= b.avail("out")
    elif op == "ew":
        rows, C, mode = p["rows"], p["C"], p["mode"]
        assert rows >= 1 and C >= 1 and 0 <= mode <= 4 and p["lda"] >= C and p["ldo"] >= C
        assert ext(rows, p["lda"], C) <= b.avail("a") and ext(rows, p["ldo"], C) <= b.avail("out")
        assert (C if mode == 1 else ext(rows, p["ldb"], C)) <= b.avail("b") and (mode == 1 or p["ldb"] >= C)
        if b.outs["out"].alias:
            assert p["lda"] == p["ldo"]
    elif op == "upsample2x_add":
        H2, C, ld = p["H2"], p["C"], p["ld"]
        assert H2 % 2 == 0 and H2 >= 2 and C >= 1 and ld >= C
        assert ext(H2 * H2, ld, C) <= min(b.avail("lat"), b.avail("out")) and ext((H2 // 2) ** 2, ld, C) <= b.avail("top")
    elif op == "pixel_shuffle_add":
        W, Co = p["W"], p["Co"]
        assert W >= 1 and Co >= 1 and p["ldg"] >= 4 * Co and p["ldf"] >= Co and p["ldo"] >= Co
        assert ext(W * W, p["ldg"], 4 * Co) <= b.avail("g") and ext(4 * W * W, p["ldf"], Co) <= b.avail("feat")
        assert ext(4 * W * W, p["ldo"], Co) <= b.avail("out")
    elif op == "im2col":
        S, k, T = p["S"], p["k"], T_of(p)
        assert S >= 1 and k >= 1 and p["stride"] >= 1 and p["pad"] >= 0 and T >= 1 and p["ld"] >= 3 * k * k
        assert 3 * S * S <= b.avail("chw") and ext(T * T, p["ld"], p["ld"]) <= b.avail("out")
        if "rowmap" in b.bufs:
            rm = b.bufs["rowmap"]
            assert rm.dtype == torch.int32 and rm.numel() == T * T and int(rm.min()) >= 0 and int(rm.max()) < T * T
            assert len(set(rm.tolist())) == T * T              # two tokens on one destination row would race
    elif op == "sam_preprocess":
        h, w, S = p["h"], p["w"], p["S"]
        assert h >= 1 and w >= 1 and S >= 1 and h * w * 3 <= b.avail("img") and 3 * S * S <= b.avail("out")
    elif op == "mask_resize_or":
        m, h, w, n, col0, ld = p["m"], p["h"], p["w"], p["n"], p["col0"], p["ld"]
        assert m >= 1 and h >= 1 and w >= 1 and n >= 1 and col0 >= 0 and col0 + n <= ld
        assert ext(m * m, ld, col0 + n) <= b.avail("low") and col0 + n <= b.avail("score")
        assert h * w <= b.avail("acc") and n * h * w <= b.avail("logits")
        assert bool(torch.isfinite(b.bufs["score"][col0: col0 + n]).all())
    elif op == "gather_rows":
        n, H, n_in = p["n"], p["H"], p["n_in"]
        assert n >= 1 and H >= 8 and H % 8 == 0 and b.aligned16("in") and b.aligned16("out")
        rows = b.bufs["rows"]
        assert rows.dtype == torch.int32 and rows.numel() == n and int(rows.min()) >= 0 and int(rows.max()) < n_in
        assert n_in * H * 2 <= b.avail("in") * b.itemsize("in") and n * H * 2 <= b.avail("out") * b.itemsize("out")
    else:
        raise KeyError(op)


# ================================================================================================ the C ABI call
def entry(case: Case) -> str:
    return "sr_op_" + case.op + ("_f32" if case.storage == "f32" and case.op in F32_ENTRY else "")


def abi_args(b: Built, logits=True):
    """the argument list of the entry point without the stream: buffer names as ``("buf", name)`` (``None`` = NULL), the rest by value"""
    p, op = b.p, b.case.op
    B = lambda n: ("buf", n)
    if op == "layernorm":
        return [B("x"), p["ldx"], B("w"), B("b"), B("out"), p["ldo"], p["rows"], p["C"], ("float", p["eps"])]
    if op == "transpose":
        return [B("in"), p["ld_in"], p["rows"], p["cols"], B("out"), p["ld_out"]]
    if op == "maxpool_win":
        return [B("in"), p["ld_in"], p["C"], p["n_win"], p["ws"], B("out"), p["ld_out"]]
    if op == "ew":
        return [B("a"), p["lda"], B("b"), p["ldb"], B("out"), p["ldo"], p["rows"], p["C"], p["mode"]]
    if op == "upsample2x_add":
        return [B("lat"), B("top"), B("out"), p["H2"], p["C"], p["ld"]]
    if op == "pixel_shuffle_add":
        return [B("g"), p["ldg"], B("feat"), p["ldf"], B("out"), p["ldo"], p["W"], p["Co"]]
    if op == "im2col":
        return [B("chw"), p["S"], p["k"], p["stride"], p["pad"], B("out"), p["ld"], B("rowmap") if "rowmap" in b.bufs else None]
    if op == "sam_preprocess":
        return [B("img"), p["h"], p["w"], B("out"), p["S"]]
    if op == "mask_resize_or":
        return [B("low"), p["ld"], p["col0"], p["n"], p["m"], B("score"), B("acc"), B("logits") if logits else None, p["h"], p["w"]]
    if op == "gather_rows":
        return [B("in"), B("rows"), B("out"), p["n"], p["H"]]
    raise KeyError(op)


# ================================================================================================ the case table
def _up(x, a):
    return (x + a - 1) // a * a


def _table():
    t = []
    add = lambda name, op, st, kernel, seed_name="", **p: t.append(Case(name, op, st, kernel, p, seed_name))
    # ---- layernorm, bf16: every kernel at both ends of its span, rows 1 / 7 / 9 / 17 (partial waves of the 2-rows-per-wave form, partial blocks)
    V = "k_layernorm_v<%s>"
    for C, ldo, rows, kern in ((8, 64, 17, "32,1"), (144, 192, 9, "32,1"), (256, 256, 7, "32,1"), (264, 320, 9, "64,1"), (512, 512, 1, "64,1"),
                               (520, 576, 7, "64,2"), (1024, 1024, 17, "64,2"), (1032, 1032, 9, "64,3"), (1152, 1152, 17, "64,3")):
        add(f"ln_bf16_C{C}_ldo{ldo}_r{rows}", "layernorm", "bf16", V % kern, rows=rows, C=C, ldx=_up(C, 8) + 8, ldo=ldo)
    add("ln_bf16_scalar_C100_ld128", "layernorm", "bf16", "k_layernorm<bf16_t>", rows=9, C=100, ldx=128, ldo=128)
    # the same logical input as ln_bf16_C144_ldo192_r9, through a base pointer 2 elements off: everything else vector-legal
    add("ln_bf16_scalar_by_offset_C144", "layernorm", "bf16", "k_layernorm<bf16_t>", seed_name="ln_bf16_C144_ldo192_r9", rows=9, C=144, ldx=152, ldo=192, x_off=2)
    add("ln_bf16_constant_rows", "layernorm", "bf16", V % "32,1", rows=7, C=144, ldx=192, ldo=192, input="constant")
    add("ln_bf16_scalar_constant_rows", "layernorm", "bf16", "k_layernorm<bf16_t>", rows=7, C=100, ldx=128, ldo=128, input="constant")
    add("ln_bf16_mean100", "layernorm", "bf16", V % "32,1", rows=9, C=256, ldx=256, ldo=256, input="mean100")
    add("ln_bf16_scalar_mean100", "layernorm", "bf16", "k_layernorm<bf16_t>", rows=9, C=256, ldx=256, ldo=256, input="mean100", x_off=2)
    # in place as socioreasoner_amd/sam2.py calls it: the mask decoder's token / key norms (C = ld = 256) and the upscaling norm (C = ld = 64)
    add("ln_bf16_inplace_C256", "layernorm", "bf16", V % "32,1", rows=17, C=256, ldx=256, ldo=256, inplace=1)
    add("ln_bf16_inplace_C64", "layernorm", "bf16", V % "32,1", rows=9, C=64, ldx=64, ldo=64, inplace=1)
    for C in (1, 63, 64, 65, 1152):
        add(f"ln_f32_C{C}", "layernorm", "f32", "k_layernorm<float>", rows=9 if C < 1152 else 5, C=C, ldx=_up(C, 4) + 4, ldo=min(_up(C, 4) + 8, 1152))
    add("ln_f32_mean100", "layernorm", "f32", "k_layernorm<float>", rows=9, C=256, ldx=256, ldo=256, input="mean100")
    add("ln_f32_inplace_C256", "layernorm", "f32", "k_layernorm<float>", rows=7, C=256, ldx=256, ldo=256, inplace=1)
    # ---- transpose
    for rows in (8, 13, 64, 69):
        for cols in (8, 72):
            add(f"tr_vec_{rows}x{cols}", "transpose", "bf16", "k_transpose_v", rows=rows, cols=cols, ld_in=cols + 8, ld_out=_up(rows, 8) + 8)
    add("tr_scalar_31x33", "transpose", "bf16", "k_transpose", rows=31, cols=33, ld_in=35, ld_out=40)
    add("tr_scalar_cols12", "transpose", "bf16", "k_transpose", rows=16, cols=12, ld_in=16, ld_out=24)
    add("tr_scalar_by_offset_13x72", "transpose", "bf16", "k_transpose", seed_name="tr_vec_13x72", rows=13, cols=72, ld_in=80, ld_out=24, out_off=2)
    add("tr_scalar_by_offset_69x72", "transpose", "bf16", "k_transpose", seed_name="tr_vec_69x72", rows=69, cols=72, ld_in=80, ld_out=80, out_off=2)
    # ---- maxpool_win
    for st, combos in (("bf16", ((2, 1, 1), (2, 3, 257), (4, 1, 256), (4, 3, 1), (8, 1, 257), (8, 3, 256))), ("f32", ((2, 1, 256), (4, 3, 257), (8, 1, 1)))):
        for ws, n_win, C in combos:
            add(f"mp_{st}_ws{ws}_n{n_win}_C{C}", "maxpool_win", st, "k_maxpool_win", ws=ws, n_win=n_win, C=C, ld_in=C + 5, ld_out=C + 3)
        add(f"mp_{st}_all_negative", "maxpool_win", st, "k_maxpool_win", ws=4, n_win=3, C=257, ld_in=262, ld_out=260, negative=1)
    # ---- ew: rows * C = 255 / 256 / 257 around the 256-thread block, three different leading dimensions, in place on a
    for st in ("bf16", "f32"):
        for mode in range(5):
            for rows, C, inplace in ((15, 17, 0), (16, 16, 1), (1, 257, 0), (3, 300, 0)):
                add(f"ew_{st}_mode{mode}_{rows}x{C}" + ("_inplace" if inplace else ""), "ew", st, "k_ew", rows=rows, C=C, mode=mode,
                    lda=C + 1, ldb=C + 2, ldo=C + 1 if inplace else C + 3, inplace=inplace)
    # ---- upsample2x_add, pixel_shuffle_add
    for st in ("bf16", "f32"):
        for H2 in (2, 6):
            for C in (1, 300):
                add(f"up_{st}_H{H2}_C{C}", "upsample2x_add", st, "k_upsample2x_add", H2=H2, C=C, ld=C + 4)
        for W in (1, 3, 5):
            for Co in (1, 8, 65):
                add(f"ps_{st}_W{W}_Co{Co}", "pixel_shuffle_add", st, "k_pixel_shuffle_add", W=W, Co=Co, ldg=4 * Co + 4, ldf=Co + 2, ldo=Co + 5)
    # ---- im2col: (8,7,4,3) the product's; (9,3,2,1) a floor in the token count; (8,1,1,0); (16,11,4,5) 363 columns, a thread loop past 256
    for S, k, stride, pad in ((8, 7, 4, 3), (9, 3, 2, 1), (8, 1, 1, 0), (16, 11, 4, 5)):
        for st in ("bf16", "f32"):
            add(f"im_{st}_S{S}_k{k}_exact_ld", "im2col", st, "k_im2col", S=S, k=k, stride=stride, pad=pad, ld=3 * k * k, rowmap=0)
            add(f"im_{st}_S{S}_k{k}_ld64_rowmap", "im2col", st, "k_im2col", S=S, k=k, stride=stride, pad=pad, ld=_up(3 * k * k, 64), rowmap=1)
    # ---- sam_preprocess: down- and upscales, the identity, a 1 x 1 image; S * S = 400 / 1024 / 2304 / 4096
    for st in ("bf16", "f32"):
        for h, w, S in ((37, 53, 64), (64, 64, 64), (3, 200, 32), (90, 20, 48), (1, 1, 20)):
            add(f"pre_{st}_{h}x{w}_S{S}", "sam_preprocess", st, "k_sam_preprocess", h=h, w=w, S=S)
    # ---- mask_resize_or
    M = lambda name, m, h, w, n, col0, ld, **kw: add(name, "mask_resize_or", "f32", "k_mask_resize_or", m=m, h=h, w=w, n=n, col0=col0, ld=ld, **kw)
    M("mr_16_47x61_n3_c1_ld16", 16, 47, 61, 3, 1, 16)
    M("mr_8_8x8_identity_n1_c0_ld4", 8, 8, 8, 1, 0, 4)
    M("mr_16_5x130_n3_c0_ld4", 16, 5, 130, 3, 0, 4)
    M("mr_32_96x96_n3_c1_ld16", 32, 96, 96, 3, 1, 16)
    M("mr_32_96x96_blob_n3_c1_ld4", 32, 96, 96, 3, 1, 4, input="blob")
    M("mr_16_47x61_tie_n3_c1_ld16", 16, 47, 61, 3, 1, 16, tie=1)
    M("mr_16_47x61_tie_n2_c0_ld4", 16, 47, 61, 2, 0, 4, tie=1)
    M("mr_16_47x61_zero_map", 16, 47, 61, 3, 1, 16, input="zero")
    # ---- gather_rows: H / 8 = 1, 8, 257 16-byte chunks per row (257 > the block's 256 threads)
    for n in (1, 5):
        for H in (8, 64, 2056):
            add(f"ga_bf16_n{n}_H{H}", "gather_rows", "bf16", "k_gather_rows", n=n, H=H, n_in=7)
    add("ga_f32_n5_H72", "gather_rows", "f32", "k_gather_rows", n=5, H=72, n_in=7)
    add("ga_f32_n5_H4112", "gather_rows", "f32", "k_gather_rows", n=5, H=4112, n_in=4)
    return tuple(t)


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the vector / scalar twins: the same logical input through both kernels
TWINS = (("ln_bf16_C144_ldo192_r9", "ln_bf16_scalar_by_offset_C144"), ("tr_vec_13x72", "tr_scalar_by_offset_13x72"),
         ("tr_vec_69x72", "tr_scalar_by_offset_69x72"))
