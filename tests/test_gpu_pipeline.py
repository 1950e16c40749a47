"""GPU: the drop-in surface -- InferenceStrategy.generate contract and the two-stage pipeline in synthetic mode."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cfg(tmp, resp=8, prompt=800):
    from roll.pipeline.rlvr.rlvr_config import SocioSegConfig
    return SocioSegConfig.from_dict({
        "output_dir": str(tmp), "prompt_length": prompt, "response_length": resp, "rollout_batch_size": 5, "pretrain": "synthetic:tiny",
        "actor_infer": {"model_args": {"model_name_or_path": "synthetic:tiny"},
                        "generating_args": {"max_new_tokens": resp, "temperature": 1, "top_k": 100, "top_p": 0.8, "num_beams": 1},
                        "strategy_args": {"strategy_name": "vllm", "strategy_config": {"max_batch": 4, "max_patches": 4096}}},
        "seg_infer": {"model_args": {}, "strategy_args": {"strategy_name": "seg_infer"}},
    })


def test_strategy_generate_contract(tmp_path):
    from roll.distributed.scheduler.protocol import DataProto
    from roll.distributed.strategy.factory import create_strategy
    from roll.pipeline.rlvr.rlvr_socioseg_vlm_pipeline_infer import _Worker
    from socioreasoner_amd import synthetic
    cfg = _cfg(tmp_path)
    st = create_strategy(_Worker(cfg.actor_infer, cfg, 0, 1, 0))
    st.initialize(None)
    g = st.geom
    P, pad = 800, g.pad_token_id
    prompts, payload = [], np.empty(5, dtype=object)
    for i in range(5):
        if i == 3:   # text-only row, short
            ids = np.arange(5, 25, dtype=np.int64)
            payload[i] = {"prompt_token_ids": ids.tolist()}
        else:
            ids = synthetic.tile_prompt(g, i, (1, 32, 32), n_pre=10 + i, n_post=7)
            payload[i] = {"prompt_token_ids": ids.tolist(), "multi_modal_data": {"image": [synthetic.tile_pixels(i)]}}
        row = np.full(P, pad, dtype=np.int64)
        row[P - len(ids):] = ids
        prompts.append(row)
    input_ids = torch.from_numpy(np.stack(prompts))
    batch = DataProto(batch={"input_ids": input_ids, "attention_mask": (input_ids != pad).long()},
                      non_tensor_batch={"multi_modal_data": payload})
    gc = {"max_new_tokens": 8, "temperature": 0, "top_p": 1.0, "top_k": 1, "num_beams": 1, "repetition_penalty": 1.0,
          "num_return_sequences": 1, "eos_token_id": [g.eos_token_id], "pad_token_id": pad}
    out = st.generate(batch, gc)
    assert out.shape[0] == 5 and P < out.shape[1] <= P + 8 and out.dtype == torch.long
    assert torch.equal(out[:, :P], input_ids)                       # prompt part verbatim (left padded)
    # batch composition must not change a sequence: row 2 alone gives the same response
    single = DataProto(batch={"input_ids": input_ids[2:3], "attention_mask": (input_ids[2:3] != pad).long()},
                       non_tensor_batch={"multi_modal_data": payload[2:3]})
    out1 = st.generate(single, gc)
    L = min(out.shape[1], out1.shape[1])
    assert torch.equal(out1[0, P:L], out[2, P:L])
    # one placeholder per image (vLLM-style prompt) expands to the same ids
    ids = np.asarray(payload[0]["prompt_token_ids"])
    keep = np.ones(len(ids), dtype=bool)
    first = int(np.argmax(ids == g.image_token_id))
    keep[first + 1: first + 256] = False
    payload2 = np.empty(1, dtype=object)
    payload2[0] = {"prompt_token_ids": ids[keep].tolist(), "multi_modal_data": payload[0]["multi_modal_data"]}
    out2 = st.generate(DataProto(batch={"input_ids": input_ids[0:1], "attention_mask": (input_ids[0:1] != pad).long()},
                                 non_tensor_batch={"multi_modal_data": payload2}), gc)
    L = min(out.shape[1], out2.shape[1])
    assert torch.equal(out2[0, P:L], out[0, P:L])
    # eos stops a sequence and the tail is pad
    first_tok = int(out[1, P])
    gc2 = dict(gc, eos_token_id=[first_tok])
    out3 = st.generate(batch, gc2)
    assert int(out3[1, P]) == first_tok and (out3[1, P + 1:] == pad).all()
    st.engine.close()


def test_pipeline_runs_two_stages_in_synthetic_mode(tmp_path, monkeypatch):
    """Real engine (synthetic tiny weights), offline stand-ins for data / tokenizer / SAM2: the reference's whole run()
    sequence executes and writes the reference's files.  Random weights emit no <answer>, so the masks are empty and the
    score is the empty-prediction IoU against the synthetic ground truth."""
    from roll.pipeline.rlvr.rlvr_socioseg_vlm_pipeline_infer import SocioSegInferPipeline, compute_giou
    monkeypatch.setenv("SOCIOSEG_NUM_SAMPLES", "3")
    cfg = _cfg(tmp_path, resp=4, prompt=1600)          # byte-level stand-in tokenizer: ~1.1k prompt tokens
    pipe = SocioSegInferPipeline(cfg)
    acc = pipe.run()
    res = os.path.join(str(tmp_path), "result")
    assert open(os.path.join(res, "iou_acc.txt")).read() == f"giou_acc: {acc}"
    for sub in ("stage1", "stage2", "render1", "render2"):
        assert len([f for f in os.listdir(os.path.join(res, sub)) if f.endswith(".png")]) == 3, sub
    assert len([f for f in os.listdir(os.path.join(res, "stage2")) if f.endswith(".txt")]) == 3
    assert acc == 0.0                                                   # empty prediction vs non-empty ground truth
    assert compute_giou(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)) == 1.0
    pipe.actor_infer.strategy.engine.close()


def _canned_boxes(question: str):
    import zlib
    rng = np.random.default_rng(zlib.crc32(question.encode()))
    out = []
    for _ in range(int(rng.integers(1, 4))):
        x0, y0 = (int(v) for v in rng.integers(0, 500, 2))
        out.append([x0, y0, x0 + int(rng.integers(3, 250)), y0 + int(rng.integers(3, 250))])
    return out


def _scripted_worker(cfg, geom, proc, seen):
    """An ActorWorker whose strategy answers from a script (a function of the prompt text): stage 1 returns canned boxes (+ malformed
    objects, one malformed JSON), stage 2 adds two points per box that was found."""
    import json
    import queue
    import re
    from roll.distributed.strategy.mi355x_strategy import Mi355xStrategy
    from roll.pipeline.base_worker import ActorWorker
    from socioreasoner_amd import hostops

    class Scripted(Mi355xStrategy):
        geom_ = geom

        def initialize(self, model_provider=None):
            self.command_queue, self.tokenizer, self.geom = queue.Queue(), proc.tokenizer, geom

        def generate(self, batch, generation_config):
            tok = self.tokenizer
            rows = []
            for payload in batch.non_tensor_batch["multi_modal_data"]:
                text = tok.decode(payload["prompt_token_ids"])
                assert text.count("<|image_pad|>") == 2 and len(payload["multi_modal_data"]["image"]) == 2
                if "have been rendered" in text:                       # stage 2: add points to the boxes that were found
                    q = re.search(r'segmentation for "(.*?)" have been rendered', text).group(1)
                    found = re.search(r"The found bbox\(s\) are: (.*?)\.Please add some points", text, re.DOTALL).group(1)
                    assert all(isinstance(im, torch.Tensor) and im.is_cuda for im in payload["multi_modal_data"]["image"])   # N3: no host round trip
                    seen["stage2_images"][q] = [im.cpu().numpy() for im in payload["multi_modal_data"]["image"]]
                    seen["stage2_text"][q] = found
                    try:
                        objs = [{"bbox_2d": o["bbox_2d"], "points": [[(o["bbox_2d"][0] + o["bbox_2d"][2]) // 2, (o["bbox_2d"][1] + o["bbox_2d"][3]) // 2],
                                                                       [o["bbox_2d"][2] + 15, o["bbox_2d"][3] + 15]]} for o in json.loads(found)
                                if isinstance(o, dict) and len(o.get("bbox_2d", [])) == 4]
                        ans = json.dumps(objs)
                    except Exception:
                        ans = "[]"
                    resp = f"<think>refine</think>\n<answer>{ans}</answer><|im_end|>"
                else:
                    q = re.search(r"Please find '(.*?)' with bboxs", text).group(1)
                    if q == "school":                                   # malformed JSON: the whole sample parses to no prompt
                        resp = "<think>x</think><answer>[{\"bbox_2d\": [1,2,3</answer><|im_end|>"
                    else:
                        objs = [{"bbox_2d": b} for b in _canned_boxes(q)] + [{"bbox_2d": [1, 2, 3]}, "junk"]
                        resp = f"<think>look</think><answer>{json.dumps(objs)}</answer><|im_end|>"
                rows.append(tok.encode(resp))
            ids = batch.batch["input_ids"]
            out = hostops.gather_outputs_to_pad_tensor(rows, generation_config["pad_token_id"], device=ids.device)
            return hostops.concatenate_input_and_output(ids, out, 1)

        def start_server(self, data, request_complete_callback):
            """the request loop of the streamed pipeline (GenerateScheduler.open_stream): every ADD is answered from the same script"""
            from roll.distributed.scheduler.protocol import DataProto
            while True:
                command, req = self.command_queue.get()
                name = getattr(command, "name", command)
                if name == "STOP":
                    return
                if name == "ADD":
                    gc = req.meta_info["generation_config"]
                    row = self.generate(req, gc)[0, req.batch["input_ids"].shape[1]:].tolist()
                    res = DataProto(meta_info=dict(req.meta_info))
                    res.meta_info["output_token_ids"] = [[int(t) for t in row if int(t) != int(gc["pad_token_id"])]]
                    seen.setdefault("streamed_requests", []).append(int(req.meta_info["request_id"]))
                    request_complete_callback(data=res)

    w = ActorWorker(cfg.actor_infer, cfg, 0, 1, 0, "actor_infer")
    w.strategy = Scripted(w)
    w.strategy.initialize()
    return w


@pytest.mark.parametrize("streamed", [True, False])
def test_pipeline_two_stage_flow_against_oracle(tmp_path, monkeypatch, streamed):
    """The reference's run() sequence with a scripted LM (answers are a function of the prompt text): parsing, SAM-prompt
    construction, union / nearest resize, render onto both images, stage-2 prompt construction and IoU are compared with
    the oracle restatements step by step (device raster kernels vs numpy / C).  Both orders of the host flow: the reference's
    (two generate calls per batch, SOCIOSEG_STREAM=0) and the streamed one (one open request stream, a sample's stage-2 prompt
    added as soon as its stage-1 answer is segmented) must write the same files and the same score."""
    monkeypatch.setenv("SOCIOSEG_STREAM", "1" if streamed else "0")
    monkeypatch.setenv("SOCIOSEG_COLLATE_CHUNK", "3")          # streamed: the batch of 4 is collated as 3 + 1 rows, the first piece on the engine before the second exists
    import json
    import queue
    import re
    from oracle import host_ref as H
    from roll.distributed.strategy.mi355x_strategy import Mi355xStrategy
    from roll.pipeline.base_worker import ActorWorker
    from roll.pipeline.rlvr import rlvr_socioseg_vlm_pipeline_infer as P
    from socioreasoner_amd import hostops, socioseg_data
    from socioreasoner_amd.config import geometry_tiny
    from socioreasoner_amd.textproc import SyntheticProcessor
    geom = geometry_tiny()
    proc = SyntheticProcessor(geom)
    cfg = _cfg(tmp_path, resp=400, prompt=2200)
    cfg.actor_infer.generating_args["temperature"] = 0
    cfg["rollout_batch_size"] = 3          # two rollout batches (3 + 1 samples): the streamed order starts the second while the first is still in stage 2
    seen = {"stage2_images": {}, "stage2_text": {}}

    w = _scripted_worker(cfg, geom, proc, seen)
    samples = socioseg_data.synthetic_socioseg(4)
    pipe = P.SocioSegInferPipeline(cfg, dataset=samples, processor=proc, actor_worker=w)
    acc = pipe.run()
    res = os.path.join(str(tmp_path), "result")
    # ---- oracle replay
    sam = socioseg_data.SyntheticSamPredictor()
    want_iou = []
    from PIL import Image
    for s in samples:
        q = s["problem"]
        sam.set_image(Image.new("RGB", (756, 756)))

        def masks_for(prompts):
            acc_m = np.zeros((756, 756), np.uint8)
            for pr in prompts:
                m, sc, _ = sam.predict(**pr)
                acc_m = H.mask_union([acc_m, m[int(np.argmax(sc))].astype(np.uint8)])
            return H.resize_nearest(acc_m, 768, 768)
        boxes1 = [] if q == "school" else _canned_boxes(q)
        mask1 = masks_for([{"box": np.array(b)} for b in boxes1])
        got1 = np.asarray(Image.open(os.path.join(res, "stage1", s["id"] + ".png")))
        assert np.array_equal(got1, mask1 * 255), s["id"]
        # the stage-2 prompt embeds the stage-1 answer text verbatim; the images are the rendered (map, sat) pair
        ans1 = "" if q == "school" else json.dumps([{"bbox_2d": b} for b in boxes1] + [{"bbox_2d": [1, 2, 3]}, "junk"])
        if q == "school":
            ans1 = '[{"bbox_2d": [1,2,3'
        assert seen["stage2_text"][q] == ans1
        for k, key in enumerate(("map_image", "sat_image")):
            base = np.asarray(P.process_image([s[key].convert("RGB")], proc)[0])
            draw = [b for b in boxes1] if q != "school" else []
            want_img = H.render_overlay(base, H.resize_nearest(mask1, base.shape[0], base.shape[1]), draw)
            assert np.array_equal(seen["stage2_images"][q][k], want_img), (s["id"], key)
        pr2 = []
        for b in boxes1:
            pr2.append({"box": np.array(b), "point_coords": np.array([[(b[0] + b[2]) // 2, (b[1] + b[3]) // 2], [b[2] + 15, b[3] + 15]]),
                        "point_labels": np.array([1, 1])})
        mask2 = masks_for(pr2)
        got2 = np.asarray(Image.open(os.path.join(res, "stage2", s["id"] + ".png")))
        assert np.array_equal(got2, mask2 * 255), s["id"]
        want_iou.append(H.compute_giou(mask2, np.asarray(s["mask_label"].convert("L"))))
        assert "<answer>" in open(os.path.join(res, "stage2", s["id"] + ".txt")).read()
    assert abs(acc - float(np.mean(want_iou))) < 1e-12 and acc > 0
    assert open(os.path.join(res, "iou_acc.txt")).read() == f"giou_acc: {acc}"
    assert pipe.streamed == streamed
    if streamed:       # every sample went through the ONE open stream twice: batch 0 owns ids 0..2 (stage 1) and 3..5 (stage 2), batch 1 ids 6 and 7; a sample's stage 2 after its stage 1
        order = seen["streamed_requests"]
        assert sorted(order) == list(range(8)) and all(order.index(i) < order.index(3 + i) for i in range(3)) and order.index(6) < order.index(7), order
    else:
        assert "streamed_requests" not in seen


def test_checkpoint_loader_safetensors_both_namings(tmp_path):
    """sr_load_weight through an HF-style *.safetensors directory (reference-era AND transformers-5 parameter names,
    bf16 and fp32 tensors, lm_head.weight present) gives the same engine as the device-side synthetic generator."""
    from safetensors.torch import save_file
    from oracle import weights as WG
    from oracle import model_ref as MR
    from socioreasoner_amd import synthetic
    from socioreasoner_amd.config import geometry_tiny
    from socioreasoner_amd.engine import Engine
    geom, cfg = geometry_tiny(), MR.config_tiny()
    W = WG.LazyWeights(cfg, seed=0)
    shard1, shard2 = {}, {}
    for i, (name, shape, base) in enumerate(WG.param_specs(cfg)):
        t = W[name].clone()
        new = name
        if i % 2 == 0:      # transformers-5 naming for every other tensor
            new = name.replace("visual.", "model.visual.", 1) if name.startswith("visual.") else name.replace("model.", "model.language_model.", 1)
        t = t.to(torch.bfloat16) if i % 3 else t.float()
        (shard1 if i % 2 else shard2)[new] = t.contiguous()
    shard2["lm_head.weight"] = W["model.embed_tokens.weight"].to(torch.bfloat16).contiguous()
    save_file(shard1, str(tmp_path / "model-00001-of-00002.safetensors"))
    save_file(shard2, str(tmp_path / "model-00002-of-00002.safetensors"))
    kw = dict(max_patches=256, max_prefill_tokens=128, max_batch=1, max_ctx=128, max_new_tokens=8)
    a, b = Engine(geom, **kw), Engine(geom, **kw)
    a.load_synthetic_weights(seed=0)
    b.load_safetensors_dir(str(tmp_path))
    img = torch.from_numpy(synthetic.tile_pixels(3, 112, 84)).cuda()
    grid = [(1, 8, 6)]
    ea, eb = a.vit_forward(a.patchify(img), grid), b.vit_forward(b.patchify(img), grid)
    assert torch.equal(ea, eb)
    ids = synthetic.tile_prompt(geom, 3, grid[0], n_pre=5, n_post=6)
    from socioreasoner_amd import hostops
    pos3, _ = hostops.get_rope_index(torch.from_numpy(ids)[None], grid, None, image_token_id=geom.image_token_id,
                                     vision_start_token_id=geom.vision_start_token_id)
    la = a.prefill([ids], [pos3[:, 0].numpy()], ea, return_logits=True)
    lb = b.prefill([ids], [pos3[:, 0].numpy()], eb, return_logits=True)
    assert torch.equal(la, lb) and torch.equal(a.decode(8), b.decode(8))
    # a missing tensor is reported, not silently zero
    c = Engine(geom, **kw)
    with pytest.raises(Exception, match="missing"):
        c.load_state_dict({k: v for k, v in shard1.items()})
    for e in (a, b, c):
        e.close()


def test_strategy_sampling_path():
    """temperature / top_k / top_p requests go token by token through sr_decode_step: top_k=1 is the greedy path bit for
    bit; a sampled run is reproducible under the same seed, respects top_k's support and yields n distinct rows."""
    from roll.distributed.scheduler.protocol import DataProto
    from roll.distributed.strategy.factory import create_strategy
    from socioreasoner_amd.config import geometry_tiny
    geom = geometry_tiny()

    class W:   # minimal worker
        rank, world_size = 0, 1
        pipeline_config = type("P", (), {"prompt_length": 64, "response_length": 16})()
        worker_config = type("C", (), {"strategy_args": type("S", (), {"strategy_name": "mi355x", "strategy_config": {"max_batch": 4, "max_ctx": 128}})(),
                                       "model_args": type("M", (), {"model_name_or_path": "synthetic:tiny"})()})()
        rank_info = type("R", (), {"local_rank": 0})()
    st = create_strategy(W())
    st.initialize(None)
    rng = np.random.default_rng(5)
    P = 24
    ids = torch.from_numpy(rng.integers(0, 2000, size=(3, P))).long()
    mask = torch.ones(3, P, dtype=torch.long)
    ids[1, :7] = geom.pad_token_id if geom.pad_token_id < 2040 else 0
    mask[1, :7] = 0
    batch = DataProto(batch={"input_ids": ids, "attention_mask": mask}, non_tensor_batch={})
    base = dict(max_new_tokens=12, eos_token_id=[2046], pad_token_id=2045, num_beams=1, num_return_sequences=1, repetition_penalty=1.0)
    greedy = st.generate(batch, dict(base, temperature=0.0, top_p=1.0, top_k=-1))
    k1 = st.generate(batch, dict(base, temperature=0.9, top_p=0.95, top_k=1))
    assert torch.equal(greedy, k1)
    # force the step-wise path with a sampler that is still deterministic: repetition_penalty != 1 at temperature 0
    # cannot be compared to greedy, but temperature -> tiny with top_k 2 must pick one of the two best tokens each step
    st._generator = None
    a = st.generate(batch, dict(base, temperature=0.8, top_p=0.9, top_k=5, seed=11, num_return_sequences=2))
    st._generator = None
    b = st.generate(batch, dict(base, temperature=0.8, top_p=0.9, top_k=5, seed=11, num_return_sequences=2))
    assert a.shape[0] == 6 and torch.equal(a, b)
    assert torch.equal(a[:, :P], ids.repeat_interleave(2, dim=0))
    assert not torch.equal(a[0::2], a[1::2])                    # the two samples of a prompt differ somewhere
    # top_k = 2: every sampled token is among the two most likely of the engine's own logits (checked by replay)
    st._generator = None
    c = st.generate(batch, dict(base, temperature=1.5, top_p=1.0, top_k=2, seed=3))
    eng = st.engine
    from socioreasoner_amd import hostops
    prompts = hostops.gather_unpadded_input_ids(ids, mask)
    pos = [np.tile(np.arange(len(p)), (3, 1)) for p in prompts]
    lg = eng.prefill([np.asarray(p) for p in prompts], pos, None, return_logits=True)
    for i in range(12):
        tok = c[:, P + i].cuda()
        top2 = lg.topk(2, dim=-1).indices
        assert bool(((tok[:, None] == top2).any(-1)).all()), i
        lg, _ = eng.decode_step(tok)


def test_request_level_serving_on_the_engine():
    """generate_opt_level 1 on the real engine: single-prompt requests through add_request / start_server (continuous
    batching) return the tensors of the batch call (level 0)."""
    from roll.distributed.scheduler.generate_scheduler import GenerateScheduler
    from roll.distributed.scheduler.protocol import DataProto
    from roll.pipeline.base_worker import ActorWorker
    from socioreasoner_amd import synthetic
    cfg = _cfg("/tmp/unused", resp=12, prompt=400)
    cfg.actor_infer.generating_args.update({"temperature": 0, "top_k": 1, "max_new_tokens": 12})
    cfg.actor_infer.strategy_args.strategy_config["max_batch"] = 3
    w = ActorWorker(cfg.actor_infer, cfg, 0, 1, 0, "actor_infer").initialize(cfg)
    g = w.strategy.geom
    P, pad = 400, g.pad_token_id
    rows, payload = [], np.empty(7, dtype=object)
    for i in range(7):
        if i % 3 == 1:
            ids = np.arange(5, 25 + i, dtype=np.int64)
            payload[i] = {"prompt_token_ids": ids.tolist()}
        else:
            ids = synthetic.tile_prompt(g, i, (1, 16, 16), n_pre=6 + i, n_post=5)
            payload[i] = {"prompt_token_ids": ids.tolist(), "multi_modal_data": {"image": [synthetic.tile_pixels(i, 224, 224)]}}
        row = np.full(P, pad, dtype=np.int64)
        row[P - len(ids):] = ids
        rows.append(row)
    input_ids = torch.from_numpy(np.stack(rows))
    mask = (input_ids != pad).long()
    pos = (mask.cumsum(-1) - 1).clamp(min=0)[:, None, :].repeat(1, 3, 1)

    def fresh():
        return DataProto(batch={"input_ids": input_ids.clone(), "attention_mask": mask.clone(), "position_ids": pos.clone()},
                         non_tensor_batch={"multi_modal_data": payload.copy()})
    sched = GenerateScheduler()
    out0 = sched.generate(fresh(), w, cfg)
    cfg["generate_opt_level"] = 1
    out1 = sched.generate(fresh(), w, cfg)
    for k in ("responses", "input_ids", "attention_mask", "response_mask", "position_ids"):
        assert torch.equal(out0.batch[k], out1.batch[k]), k
    assert int(out0.batch["response_mask"].sum()) > 0
    w.strategy.engine.close()


def test_two_rank_data_parallel_bench_equals_single_process():
    """Section 8(E): two torchrun ranks (RCCL when there are two GPUs, gloo + shared GPU on a one-GPU box), one tile each,
    give the result rows of one process running both tiles; the logits all-gather verification mode agrees as well."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(cmd, port=None):
        # two ranks on the ONE GPU of the test box: sharing a device over gloo has to be asked for (dp.init_distributed refuses to
        # fall back silently; RCCL with one GPU per rank is the driver's scaling tier)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", SR_DIST_BACKEND="gloo")
        out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
        return json.loads(line)
    common = ["--full", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"]      # (--full: the roofline object checked below)
    tr = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1"]
    one = run([sys.executable, "bench.py", "--batch", "2", "--static", "--no-latency"] + common)
    two = run(tr + ["--master-port", "29551", "bench.py", "--gpus", "2", "--batch", "1"] + common)
    ver = run(tr + ["--master-port", "29552", "bench.py", "--gpus", "2", "--batch", "1", "--gather-logits"] + common)
    assert two["config"]["exchange"]["backend"] == "gloo" and two["config"]["exchange"]["nranks"] == 2
    assert two["n_gpus"] == 2 and two["config"]["parallelism"] == "dp2" and two["scaling"] == "weak"
    assert one["result_checksum"] == two["result_checksum"] == ver["result_checksum"]
    for j in (one, two):
        assert j["roofline"]["bound"] == "hbm" and 0 < j["roofline"]["frac"] < 1 and j["unit"] == "tiles/s"


@pytest.mark.parametrize("fp8", [False, True])
def test_weight_sync_into_the_engine(fp8):
    """N4: an engine whose weights arrive through the reference's bucket protocol (update_parameter_in_bucket, pieces split
    across 1 MB buckets, fp32 and bf16 tensors) generates exactly what an engine loaded directly generates -- also with fp8
    LM linears, where every fused matrix is re-quantised once all of its tensors have arrived; a second sync round with
    changed weights changes the output, and a partial round is refused in fp8 mode."""
    from oracle import model_ref as MR
    from oracle import weights as WG
    from roll.distributed.scheduler.protocol import DataProto
    from roll.distributed.strategy.factory import create_strategy
    from roll.pipeline.base_worker import Worker
    from socioreasoner_amd.weight_sync import BucketSender
    cfg = _cfg("/tmp/unused", resp=8, prompt=64)
    cfg.actor_infer.generating_args.update({"temperature": 0, "top_k": 1})
    if fp8:
        cfg.actor_infer.strategy_args.strategy_config["quantization"] = "fp8"
    rcfg = MR.config_tiny()
    W = WG.LazyWeights(rcfg, seed=0)
    specs = WG.param_specs(rcfg)

    def strat():
        st = create_strategy(Worker(cfg.actor_infer, cfg, 0, 1, 0))
        st.initialize(None)                       # synthetic weights, seed 0
        return st

    def sync(st, scale=1.0, only=None):
        snd = BucketSender(1 << 20, device="cuda")
        for i, (name, shape, base) in enumerate(specs):
            if only is not None and name not in only:
                continue
            t = (W[name] * scale).to(torch.bfloat16 if i % 2 else torch.float32).cuda()
            for meta, buf in snd.push(name, t):
                st.update_parameter_in_bucket({k: dict(v) for k, v in meta.items()}, buf.clone(), [0])
        meta, buf = snd.flush()
        if meta:
            st.update_parameter_in_bucket(meta, buf.clone(), [0])
    rng = np.random.default_rng(1)
    ids = torch.from_numpy(rng.integers(0, 2000, size=(2, 20))).long()
    batch = DataProto(batch={"input_ids": ids, "attention_mask": torch.ones_like(ids)}, non_tensor_batch={})
    gc = dict(max_new_tokens=8, eos_token_id=[2046], pad_token_id=2045, num_beams=1, num_return_sequences=1, repetition_penalty=1.0, temperature=0.0, top_k=1, top_p=1.0)
    a, b = strat(), strat()
    want = a.generate(batch, gc)
    b.engine.load_weight("model.norm.weight", torch.zeros(512))     # make sure the sync really overwrites
    sync(b)
    assert torch.equal(b.generate(batch, gc), want)
    sync(b, scale=1.5)
    assert not torch.equal(b.generate(batch, gc), want)
    sync(b)
    assert torch.equal(b.generate(batch, gc), want)
    if fp8:
        sync(b, only={"model.layers.0.self_attn.q_proj.weight"})
        with pytest.raises(Exception, match="partly reloaded"):
            b.generate(batch, gc)
    a.engine.close()
    b.engine.close()


def test_forward_step_all_position_logits(golden_dir=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")):
    """InferenceStrategy.forward_step (hf_strategy.py:49-94): logits at every position for left-padded (image + text,
    text-only) rows against the oracle's teacher-forced forward, zeros at padded positions, micro-batching + collation."""
    from oracle import model_ref as MR
    from oracle import weights as WG
    from roll.distributed.scheduler.protocol import DataProto
    from roll.distributed.strategy.factory import create_strategy
    from roll.pipeline.base_worker import Worker
    from tests.util import bits_to_f32
    cfg = _cfg("/tmp/unused", resp=8, prompt=160)
    st = create_strategy(Worker(cfg.actor_infer, cfg, 0, 1, 0))
    st.initialize(None)
    g = np.load(os.path.join(golden_dir, "hf_tiny.npz"))
    rcfg = MR.config_tiny()
    W = WG.LazyWeights(rcfg, seed=0)
    grids = [tuple(x) for x in g["grids"].tolist()]
    pix = bits_to_f32(g["pix"])
    ids_img, pos_img = g["ids"], g["pos3"]
    txt = np.arange(7, 30, dtype=np.int64)
    S = 160
    input_ids = torch.zeros(3, S, dtype=torch.long)
    mask = torch.zeros(3, S, dtype=torch.long)
    pos = torch.zeros(3, 3, S, dtype=torch.long)
    rows = [(ids_img, pos_img), (txt, np.tile(np.arange(len(txt)), (3, 1))), (ids_img, pos_img)]
    for i, (a, p3) in enumerate(rows):
        input_ids[i, S - len(a):] = torch.from_numpy(a)
        mask[i, S - len(a):] = 1
        pos[i, :, S - len(a):] = torch.from_numpy(p3)
    mm = np.empty(3, dtype=object)
    mm[0] = {"pixel_values": pix, "image_grid_thw": torch.tensor(grids)}
    mm[1] = {}
    mm[2] = {"pixel_values": pix, "image_grid_thw": torch.tensor(grids)}
    batch = DataProto(batch={"input_ids": input_ids, "attention_mask": mask, "position_ids": pos},
                      non_tensor_batch={"multi_modal_inputs": mm}, meta_info={"micro_batch_size": 1})
    seen = []

    def forward_func(data, logits):
        seen.append(logits.float().cpu())
        lp = torch.log_softmax(logits.float(), dim=-1)[:, :-1].gather(-1, data.batch["input_ids"][:, 1:, None].to(logits.device))[..., 0]
        lp = lp * data.batch["attention_mask"][:, 1:].to(logits.device)
        return lp.sum(), {"log_probs": lp.cpu(), "n": int(data.batch["input_ids"].shape[0])}
    res = st.forward_step(batch, forward_func)
    assert res["log_probs"].shape == (3, S - 1) and [int(x) for x in res["n"]] == [1, 1, 1]
    got = torch.cat(seen, dim=0)
    assert got.shape == (3, S, 2048)
    img_ref = MR.vit_forward(W, rcfg, pix, grids)
    for i, (a, p3) in enumerate(rows):
        x = MR.embed_with_images(W, rcfg, torch.from_numpy(a), img_ref if len(a) > 40 else None)
        ref = MR.lm_forward(W, rcfg, x, torch.from_numpy(p3), MR.new_caches(rcfg), all_logits=True)
        assert float(got[i, : S - len(a)].abs().max()) == 0.0
        d = (got[i, S - len(a):] - ref).abs()
        # bf16 noise floor of the 7-layer tiny model + the bf16 rounding of the returned logits
        assert float(d.max()) <= 0.06 and float(d.mean()) <= 0.01, (i, float(d.max()), float(d.mean()))
    assert torch.equal(got[0], got[2])
    st.engine.close()


def test_generate_decouples_admission_from_decode_and_server_survives_abort_bursts(tmp_path):
    """(1) A batch that does not fit ONE ViT / prefill admission (capacity for 2 image prompts, 4 batch rows, 7 prompts) still
    decodes at full width: generate() hands the prompts to the scheduler, every row equals the single-prompt call.
    (2) The request-level server keeps running when the same request is ABORTed repeatedly while its row is decoding
    (ROLL schedulers send ABORTs in bursts); the other requests complete, the aborted one reports nothing."""
    import queue
    import threading
    from roll.distributed.scheduler.protocol import DataProto
    from roll.distributed.strategy.factory import create_strategy
    from roll.pipeline.rlvr.rlvr_socioseg_vlm_pipeline_infer import _Worker
    from roll.utils.functionals import GenerateRequestType
    from socioreasoner_amd import synthetic
    cfg = _cfg(tmp_path, resp=12)
    cfg.actor_infer.strategy_args.strategy_config.update({"max_batch": 4, "max_patches": 2048, "max_prefill_tokens": 1000})
    st = create_strategy(_Worker(cfg.actor_infer, cfg, 0, 1, 0))
    st.initialize(None)
    g = st.geom
    P, pad = 500, g.pad_token_id
    rows, payload = [], np.empty(7, dtype=object)
    for i in range(7):
        ids = synthetic.tile_prompt(g, i, (1, 32, 32), n_pre=8 + i, n_post=6)
        payload[i] = {"prompt_token_ids": ids.tolist(), "multi_modal_data": {"image": [synthetic.tile_pixels(i)]}}
        row = np.full(P, pad, dtype=np.int64)
        row[P - len(ids):] = ids
        rows.append(row)
    input_ids = torch.from_numpy(np.stack(rows))
    gc = {"max_new_tokens": 12, "temperature": 0, "top_p": 1.0, "top_k": 1, "num_beams": 1, "repetition_penalty": 1.0,
          "num_return_sequences": 1, "eos_token_id": [g.eos_token_id], "pad_token_id": pad}

    def batch_of(sel):
        return DataProto(batch={"input_ids": input_ids[sel], "attention_mask": (input_ids[sel] != pad).long()},
                         non_tensor_batch={"multi_modal_data": payload[sel]})
    out = st.generate(batch_of(slice(0, 7)), gc)
    assert out.shape[0] == 7
    for k in (0, 3, 6):
        one = st.generate(batch_of(slice(k, k + 1)), gc)
        L = min(out.shape[1], one.shape[1])
        assert torch.equal(one[0, P:L], out[k, P:L]), k
    # ---- (2) abort bursts against running rows
    done = queue.Queue()
    err = []

    def loop():
        try:
            torch.cuda.set_device(st.engine.device)
            st.start_server(data=None, request_complete_callback=lambda data: done.put(data.meta_info["request_id"]))
        except BaseException as e:  # noqa: BLE001
            err.append(e)
    th = threading.Thread(target=loop, daemon=True)
    th.start()
    long_gc = dict(gc, max_new_tokens=12)
    for k in range(5):
        req = batch_of(slice(k, k + 1))
        req.meta_info = {"request_id": f"r{k}", "generation_config": long_gc}
        st.add_request(GenerateRequestType.ADD, req)
    import time
    time.sleep(0.05)                                  # rows are decoding now
    for _ in range(4):                                # a burst naming a running row (and once a row that never existed)
        st.add_request(GenerateRequestType.ABORT, DataProto(meta_info={"request_id": "r1"}))
    st.add_request(GenerateRequestType.ABORT, DataProto(meta_info={"request_id": "nope"}))
    st.add_request(GenerateRequestType.STOP, None)
    th.join(timeout=120)
    assert not th.is_alive() and not err, err
    got = set()
    while not done.empty():
        got.add(done.get())
    assert {"r0", "r2", "r3", "r4"} <= got and len(got) in (4, 5)      # r1 is dropped unless it finished before the burst arrived
    st.engine.close()
