"""CPU tests of beam search (num_beams > 1): the host restatement (tests/beam_ref.py) reproduces HF's recorded beam search
(tests/golden/beam_hf_tiny.npz, tools/make_golden_beam.py) exactly when fed HF's own logits; the strategy refuses the unsupported settings by
name; the C ABI declares and binds the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

from tests.beam_ref import beam_search_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "beam_hf_tiny.npz")
NAMES = ["w2_lp1_eos", "w4_lp0_2eos", "w4_lp2_maxnew"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_hf_beam_search(name):
    z = np.load(GOLD)
    W, R, max_new, pad = (int(v) for v in z[f"{name}.params"])
    lp = float(z[f"{name}.lp"][0])
    eos = z[f"{name}.eos"].tolist()
    logits = torch.from_numpy(z[f"{name}.logits"])
    ref = beam_search_ref(lambda t: logits[t], 1, W, R, max_new, eos, pad, lp, poll=1)
    assert ref["steps"] == logits.shape[0]
    seqs, bidx, scores = z[f"{name}.sequences"], z[f"{name}.beam_indices"], z[f"{name}.scores"]
    for r in range(R):
        toks, n = ref["tokens"][0][r], ref["lengths"][0][r]
        assert seqs[r, :n].tolist() == toks
        assert (seqs[r, n:] == pad).all()
        assert bidx[r, :n].tolist() == _hf_path(ref, r)        # HF's beam_indices: the beam each generated token extends
        assert (bidx[r, n:] == -1).all()
        assert abs(float(scores[r]) - ref["scores"][0][r]) <= 1e-6


def _hf_path(ref, r):
    """beam index of every generated token of finished hypothesis r: the running beam of the previous step it continues"""
    _, t, p, _ = ref["fin"][0][r]
    out = [p]
    for k in range(t - 1, -1, -1):
        p = ref["trace"][k][p][0]
        out.append(p)
    return out[::-1]


def test_fixture_covers_eos_and_max_new_endings():
    z = np.load(GOLD)
    assert os.path.getsize(GOLD) < 1 << 20
    pad = {n: int(z[f"{n}.params"][3]) for n in NAMES}
    lens = {n: (z[f"{n}.sequences"] != pad[n]).sum(1) for n in NAMES}
    assert any((lens[n] < int(z[f"{n}.params"][2])).any() for n in NAMES)      # eos ended a hypothesis early
    assert (lens["w4_lp2_maxnew"] == 8).all()
    assert len(z["w4_lp0_2eos.eos"]) == 2


@pytest.mark.parametrize("gc,word", [
    (dict(num_beams=4, repetition_penalty=1.1), "repetition_penalty"),
    (dict(num_beams=2, num_return_sequences=3), "num_return_sequences"),
    (dict(num_beams=4, early_stopping=True), "early_stopping"),
    (dict(num_beams=4, early_stopping="never"), "early_stopping"),
    (dict(num_beams=16), "num_beams"),
])
def test_strategy_refuses_unsupported_beam_settings_by_name(gc, word):
    from roll.distributed.strategy.mi355x_strategy import check_beam_config
    with pytest.raises((ValueError, NotImplementedError), match=word):
        check_beam_config(gc, 32)
    check_beam_config(dict(num_beams=4, num_return_sequences=4, length_penalty=0.5), 32)


def test_header_declares_and_lib_binds_beam_entry_points():
    from socioreasoner_amd import lib
    hdr = open(os.path.join(ROOT, "include", "socior.h")).read()
    for name in ("sr_decode_beam", "sr_op_beam_select", "sr_op_kv_suffix_copy"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in lib.SIGNATURES, name
    assert len(lib.SIGNATURES["sr_decode_beam"][1]) == 17
