"""Reference of the token log-probs the engine records (sr_logprobs): the float64 definition, the bound the float32 kernels are held to, a
float32 restatement of the kernels' chunked sum (used only to size that bound, never compared with a kernel) and the op-level test rows."""
import numpy as np

UNIT = 2.0 ** -23
CHUNK = 4096          # logits per chunk of the kernels' first pass (RS_CH)


def log_softmax64(x):
    """log_softmax of float32 logits [..., V] in float64 (-inf entries allowed, a row needs one finite entry)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def top_n(x, n):
    """ids of the n largest logits of every row, ordered by (logit descending, id ascending): a stable sort on -logit"""
    x = np.asarray(x, dtype=np.float32)
    V = x.shape[-1]
    rows = x.reshape(-1, V)
    out = np.empty((rows.shape[0], n), dtype=np.int64)
    for i, row in enumerate(rows if n else ()):
        # (only the entries at or above the n-th largest value can be among the first n of the stable sort)
        cand = np.flatnonzero(row >= np.partition(row, V - n)[V - n])
        out[i] = cand[np.argsort(-row[cand].astype(np.float64), kind="stable")][:n]
    return out.reshape(x.shape[:-1] + (n,))


def token_logprobs(x, tokens=None, n=0, ls=None):
    """the record of every row of float32 logits x [R, V]: tokens [R] (None: the arg-max, lowest id among the maxima) ->
    dict(tok int64 [R], lp float64 [R], lse float64 [R], top_ids int64 [R, n], top_lp float64 [R, n]).  ls: log_softmax64(x) when the
    caller already has it"""
    x = np.asarray(x, dtype=np.float32)
    ls = log_softmax64(x) if ls is None else ls
    r = np.arange(x.shape[0])
    am = top_n(x, 1)[:, 0]
    tok = am if tokens is None else np.asarray(tokens, dtype=np.int64)
    ids = top_n(x, n)
    with np.errstate(invalid="ignore"):
        lse = x[r, tok].astype(np.float64) - ls[r, tok]
    # (a token at -inf gives lse = nan above: take it from the row's maximum, which is finite)
    lse = np.where(np.isfinite(lse), lse, x[r, am].astype(np.float64) - ls[r, am])
    return {"tok": tok, "lp": ls[r, tok], "lse": lse, "top_ids": ids, "top_lp": np.take_along_axis(ls, ids, axis=-1)}


def bound(x_tok, lse64):
    """|lp - lp64| <= 8 x 2^-23 x max(8, |x_tok|, |lse64|): a float32 sum of at most V terms in (0, 1], two roundings at the magnitude of lse
    and x_tok, expf / logf within a few ulp (the sequential float32 restatement below stays near 1.2 of those units: about 7 x headroom)"""
    return 8 * UNIT * np.maximum(8.0, np.maximum(np.abs(x_tok), np.abs(lse64)))


def chunked_f32(x, tok):
    """lp of one float32 row as the kernels sum it, restated in float32: per chunk of 4096 the maximum and sum exp(x - max) -- 256 threads, thread t
    adds elements t, t + 256, ... in order, then the 64-lane butterfly and (w0 + w1) + (w2 + w3) -- then the chunks merged in chunk order"""
    f = np.float32
    x = np.asarray(x, dtype=f)
    ms, ss = [], []
    lanes = np.arange(64)
    for c0 in range(0, len(x), CHUNK):
        v = np.full(CHUNK, -np.inf, dtype=f)
        seg = x[c0:c0 + CHUNK]
        v[:len(seg)] = seg
        v = v.reshape(CHUNK // 256, 256)
        m = v.max()
        with np.errstate(invalid="ignore"):
            e = np.where(v == -np.inf, f(0), np.exp((v - m).astype(f)).astype(f)).astype(f)
        s = np.zeros(256, dtype=f)
        for k in range(v.shape[0]):
            s = (s + e[k]).astype(f)
        w = s.reshape(4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            w = (w + w[:, lanes ^ o]).astype(f)
        ms.append(m)
        ss.append(f(f(w[0, 0] + w[1, 0]) + f(w[2, 0] + w[3, 0])))
    M = max(ms)
    S = f(0)
    for m, s in zip(ms, ss):
        if m != -np.inf:
            S = f(S + f(s * np.exp(f(m - M)).astype(f)))
    lse = f(M + np.log(S).astype(f))
    with np.errstate(invalid="ignore"):
        return f(x[tok] - lse)


KINDS = ("normal", "wide", "plus80", "minus80", "constant", "one_finite", "dup_max", "neg_inf", "narrow_plus60", "wide_minus60")


def op_rows(V, rows, seed):
    """float32 logits [rows, V] of the op-level table, row i of kind KINDS[i % len(KINDS)]: deviations 0.5 .. 25, offsets +-60 / +-80, a constant
    row, a row with one finite entry, duplicated maxima (the lowest id must win), -inf entries"""
    rng = np.random.default_rng(seed)
    x = np.empty((rows, V), dtype=np.float32)
    kinds = []
    for i in range(rows):
        k = KINDS[i % len(KINDS)]
        kinds.append(k)
        g = rng.standard_normal(V).astype(np.float32)
        if k == "normal":
            x[i] = g * 2.5
        elif k == "wide":
            x[i] = g * 25.0
        elif k == "plus80":
            x[i] = np.clip(g * 1.5, -6, 6) + 74.0          # (magnitude 80 at most)
        elif k == "minus80":
            x[i] = np.clip(g * 1.5, -6, 6) - 74.0
        elif k == "constant":
            x[i] = np.float32(rng.uniform(-3, 3))
        elif k == "one_finite":
            x[i] = -np.inf
            x[i, int(rng.integers(0, V))] = np.float32(rng.uniform(-20, 20))
        elif k == "dup_max":
            x[i] = g
            at = np.sort(rng.choice(V, size=min(5, V), replace=False))
            x[i, at] = np.float32(7.25)                     # several maxima, far above the rest
            if V > CHUNK:
                x[i, V - 1] = np.float32(7.25)              # ... one of them in the last chunk
        elif k == "neg_inf":
            x[i] = g * 3.0
            x[i, rng.random(V) < 0.4] = -np.inf
            x[i, int(rng.integers(0, V))] = 1.0
        elif k == "narrow_plus60":
            x[i] = g * 0.5 + 60.0
        else:
            x[i] = np.clip(g * 5.0, -19, 19) - 60.0
    return x, kinds
