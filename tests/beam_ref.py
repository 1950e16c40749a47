"""Host restatement of the engine's beam search (HF GenerationMixin._beam_search with do_sample=False, early_stopping=False), in torch
float32 over a callback that supplies each step's logits.  Not a test module: tests/test_host_beam.py pins it against HF's recorded run, and
tests/test_gpu_beam.py feeds it the device's own logits trace and compares it with sr_decode_beam.

Rules (include/socior.h, sr_decode_beam): W beams per group, running scores 0, -1e9, ...; every step the top K = max(2, 1 + n_eos) * W
candidates running + log_softmax (ties: lower beam * V + token); a candidate hits on an eos token or at the max_new-th token; the next
running beams are the top W after -1e9 is added to the hits; hits among the first W enter the finished list (best W, older entries first on
equal scores) with score cum / gen_len ** lp; a group with a full list stops once best_running / gen_len ** lp <= its worst entry, and
from then on freezes (trace entries (-1, pad)).  The device polls its stop flags after steps 15, 31, ... (0-based); `poll=16` mimics that."""
import torch


def beam_search_ref(logits_fn, G, W, R, max_new, eos, pad, lp=1.0, poll=16):
    """logits_fn(t) -> float32 [G * W, V] (row g * W + j: beam j of group g at step t).  Returns a dict: trace [steps][G*W] of (parent,
    token), fin [G] lists of (score, step, parent, token), stop [G] (step or -1), steps, tokens [G][R] lists (eos included), scores [G][R],
    lengths [G][R]."""
    eos = [int(x) for x in eos]
    K = max(2, 1 + len(eos)) * W
    running = torch.full((G, W), -1.0e9, dtype=torch.float32)
    running[:, 0] = 0.0
    fin = [[] for _ in range(G)]
    done = [False] * G
    stop = [-1] * G
    trace = []
    steps = 0
    for t in range(max_new):
        lg = logits_fn(t).float()
        V = lg.shape[-1]
        logp = torch.log_softmax(lg, dim=-1)
        row = [None] * (G * W)
        denom = torch.tensor(float((t + 1) ** lp), dtype=torch.float32)
        last = t + 1 >= max_new
        for g in range(G):
            if done[g]:
                for j in range(W):
                    row[g * W + j] = (-1, pad)
                continue
            cand = (running[g][:, None] + logp[g * W:(g + 1) * W]).reshape(-1)
            _, order = torch.sort(cand, descending=True, stable=True)
            top = order[:K].tolist()
            sc = [cand[i] for i in top]                       # float32 0-d tensors
            hit = [last or (i % V) in eos for i in top]
            rs = [s + (torch.tensor(-1.0e9) if h else torch.tensor(0.0)) for s, h in zip(sc, hit)]
            rs_t = torch.stack(rs)
            _, sel = torch.sort(rs_t, descending=True, stable=True)
            sel = sel[:W].tolist()
            for k in range(W):                                # finished list: stable merge, older entries first
                if hit[k]:
                    e = ((sc[k] / denom).item(), t, top[k] // V, top[k] % V)
                    at = next((q for q, f in enumerate(fin[g]) if e[0] > f[0]), len(fin[g]))
                    fin[g].insert(at, e)
                    del fin[g][W:]
            for j, k in enumerate(sel):
                row[g * W + j] = (top[k] // V, top[k] % V)
                running[g, j] = rs[k]
            if len(fin[g]) == W and (rs[sel[0]] / denom).item() <= fin[g][-1][0]:
                done[g] = True
                stop[g] = t
        trace.append(row)
        steps = t + 1
        if t >= 1 and t % poll == poll - 1 and all(done):
            break
    tokens, scores, lengths = [], [], []
    for g in range(G):
        tg, sg, lg_ = [], [], []
        for score, t, p, tok in fin[g][:R]:
            seq = [tok]
            for k in range(t - 1, -1, -1):
                p, tk = trace[k][g * W + p]
                seq.append(tk)
            tg.append(seq[::-1])
            sg.append(score)
            lg_.append(t + 1)
        tokens.append(tg)
        scores.append(sg)
        lengths.append(lg_)
    return {"trace": trace, "fin": fin, "stop": stop, "steps": steps, "tokens": tokens, "scores": scores, "lengths": lengths}
