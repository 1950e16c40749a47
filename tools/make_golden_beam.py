#!/usr/bin/env python3
"""Generate tests/golden/beam_hf_tiny.npz: HF beam search (transformers 5.15, GenerationMixin._beam_search, do_sample=False) on the tiny
geometry in float32 with the oracle's weights.  Stores HF's inputs and outputs only: per configuration the prompt, the raw per-step logits
of every beam (output_logits), `sequences`, `sequences_scores` and `beam_indices`.  tests/test_host_beam.py feeds the logits to the host
restatement (tests/beam_ref.py) and asserts HF's sequences, beam indices and scores.

Usage: python tools/make_golden_beam.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_golden import hf_model  # noqa: E402
from oracle import model_ref as M  # noqa: E402
from oracle import weights as WG  # noqa: E402

# (name, num_beams, num_return_sequences, length_penalty, eos ranks among the prompt's first-step candidates, max_new, prompt length)
CONFIGS = [
    ("w2_lp1_eos", 2, 2, 1.0, (1,), 10, 13),         # eos (the second most likely first token) ends beams early
    ("w4_lp0_2eos", 4, 3, 0.0, (2, 5), 8, 17),       # two eos tokens: K = 3 W
    ("w4_lp2_maxnew", 4, 2, 2.0, (), 8, 11),         # no eos the beams meet: max_new ends them
]


def main():
    cfg = M.config_tiny()
    model = hf_model(cfg, WG.LazyWeights(cfg, seed=0)).to(torch.float32).eval()
    V = cfg.text.vocab_size
    out = {}
    rng = np.random.default_rng(17)
    for name, W, R, lp, eos_ranks, max_new, S in CONFIGS:
        ids = rng.integers(0, cfg.image_token_id - 8, S).astype(np.int64)
        x = torch.tensor(ids)[None]
        with torch.no_grad():
            first = model(input_ids=x, attention_mask=torch.ones_like(x)).logits[0, -1].float()
        order = torch.argsort(first, descending=True).tolist()
        eos = [int(order[r]) for r in eos_ranks] if eos_ranks else [V - 2]
        pad = V - 3
        with torch.no_grad():
            g = model.generate(input_ids=x, attention_mask=torch.ones_like(x), do_sample=False, num_beams=W, num_return_sequences=R,
                               length_penalty=lp, early_stopping=False, max_new_tokens=max_new, eos_token_id=eos, pad_token_id=pad,
                               output_logits=True, output_scores=True, return_dict_in_generate=True)
        logits = torch.stack(g.logits).float().numpy()          # [steps, W, V]
        out.update({f"{name}.ids": ids, f"{name}.logits": logits, f"{name}.sequences": g.sequences[:, S:].numpy(),
                    f"{name}.scores": g.sequences_scores.float().numpy(), f"{name}.beam_indices": g.beam_indices.numpy(),
                    f"{name}.params": np.array([W, R, max_new, pad], dtype=np.int64), f"{name}.lp": np.array([lp], dtype=np.float64),
                    f"{name}.eos": np.array(eos, dtype=np.int64)})
        print(f"{name}: steps {logits.shape[0]}, lengths {[(s != pad).sum() for s in g.sequences[:, S:].numpy()]}, scores {g.sequences_scores.tolist()}")
    path = os.path.join(ROOT, "tests", "golden", "beam_hf_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
