"""MI355X-native replacement of the reference's ``actor_infer`` strategy (roll/distributed/strategy/vllm_strategy.py)
and of the raster half of ``seg_infer`` (roll/distributed/strategy/seg_strategy.py), behind the same plugin boundary.

``Mi355xStrategy.generate`` keeps the reference contract (vllm_strategy.py:114-141):
  in : batch.batch["input_ids" | "attention_mask"] left-padded [B, P]; optionally
       batch.non_tensor_batch["multi_modal_data"][i] = {"prompt_token_ids": [...], "multi_modal_data": {"image": [PIL, ...]}}
       generation_config keys of roll/configs/generating_args.py (max_new_tokens, eos_token_id (list), pad_token_id, ...)
  out: LongTensor [B * n, P + max_response_len_in_batch]: the prompt columns verbatim, responses right-padded with pad.
Greedy requests (temperature 0 or top_k 1 -- BASELINE.json's configurations) run the whole decode loop on the device
(sr_decode, one hipGraph replay per token).  Sampling requests (the shipped YAML's temperature / top_p / top_k /
repetition_penalty, vllm_strategy.py:289-309) also stay on the device when top_k <= 1024 -- including top_k <= 0, vLLM's "no bound" (sr_decode_sample: the draw
is a kernel inside the captured step); only a top-k bound above 1024 still runs token by token through sr_decode_step with the draw
made by socioreasoner_amd.sampling on the device-resident logits.
"""
from __future__ import annotations

import contextlib
import logging
import queue
import time
from typing import Dict, List

import numpy as np
import torch

from roll.distributed.scheduler.protocol import DataProto
from roll.distributed.strategy.strategy import InferenceStrategy
from socioreasoner_amd import hostops, raster, sampling
from socioreasoner_amd.config import ModelGeometry, geometry_3b, geometry_tiny
from socioreasoner_amd.engine import Engine

logger = logging.getLogger("roll.mi355x")


class _StubTokenizer:
    """No tokenizer files are available offline: ids in, ids out.  A real run passes an HF tokenizer instead."""

    def __init__(self, geom: ModelGeometry):
        self.eos_token_id, self.pad_token_id = geom.eos_token_id, geom.pad_token_id
        self.additional_special_tokens, self.padding_side = [], "left"

    def batch_decode(self, ids, skip_special_tokens=False):
        return [" ".join(str(int(t)) for t in row if not (skip_special_tokens and int(t) == self.pad_token_id)) for row in ids]


# strategy_config device_resize when unset.  The rule: true once tools/bench_resize.py has shown, on an MI355X, the device path (upload at the source
# size + sr_resize_pil_u8) faster than the host path (PIL + upload) by more than the measured spread (profiles/device_resize.json); until then false.
DEVICE_RESIZE_DEFAULT = False


def _get(obj, name, default=None):
    if obj is None:
        return default
    if isinstance(obj, dict):
        return obj.get(name, default)
    return getattr(obj, name, default)


def _vision_quantization(sc: dict):
    """strategy_config.vision_quantization -> Engine(vit_fp8=...): unset / none / bf16 = the bf16 vision tower, fp8_mx = its linears fp8 x fp8
    on the block-scaled MFMA.  Anything else is an error by name (a typo must not silently serve bf16)."""
    v = str(sc.get("vision_quantization", "") or "").lower()
    if v in ("", "none", "bf16"):
        return False
    if v == "fp8_mx":
        return "mx"
    raise ValueError(f"strategy_config.vision_quantization {v!r}: 'fp8_mx' or unset (fp8 weights under bf16 activations have no use in the vision tower)")


class Mi355xStrategy(InferenceStrategy):
    strategy_name = "mi355x"
    request_stream = True      # start_server may stay open while prompts keep arriving (GenerateScheduler.open_stream; the two-stage pipeline's streamed mode)

    def __init__(self, worker):
        super().__init__(worker)
        self.engine: Engine | None = None
        self.command_queue: queue.Queue | None = None
        self.request_metas: Dict = {}
        self.running = False

    # ------------------------------------------------------------------ lifecycle
    def initialize(self, model_provider=None):
        sa = _get(self.worker_config, "strategy_args")
        sc = dict(_get(sa, "strategy_config", None) or {})
        margs = _get(self.worker_config, "model_args")
        path = str(_get(margs, "model_name_or_path", "") or sc.get("model", "synthetic:3b"))
        import os
        from socioreasoner_amd import checkpoints
        # the same policy as seg_infer's provider: synthetic:* | a directory | a hub id found in the local HF cache | else FileNotFoundError
        # (SR_ALLOW_SYNTHETIC_WEIGHTS=1: loud fallback to random weights of the 3B geometry)
        kind, path = checkpoints.resolve(path, "actor_infer (SocioReasoner LM)", "synthetic:3b")
        if kind == "dir" and os.path.isfile(os.path.join(path, "config.json")):    # a checkpoint directory brings its own geometry
            import json
            from socioreasoner_amd.config import geometry_from_hf_config
            self.geom = geometry_from_hf_config(json.load(open(os.path.join(path, "config.json"))))
        else:
            self.geom = geometry_tiny() if path.endswith("synthetic:tiny") else geometry_3b()
        pc = getattr(self.worker, "pipeline_config", None)
        prompt_len = int(_get(pc, "prompt_length", 4096))
        resp_len = int(_get(pc, "response_length", 2048))
        self.max_batch = int(sc.get("max_batch", 32))
        # KV cache sized for prompt + response like the reference's sequence_length (36 KB per token per slot: 32 slots x
        # 6144 tokens = 7 GB of the 288 GB)
        max_ctx = int(sc.get("max_ctx", min(prompt_len + resp_len, 8192)))
        max_ctx = (max_ctx + 63) // 64 * 64
        # ViT / prefill capacities follow the batch: the shipped workload feeds TWO images of up to 756 x 756 (2916 patches, 729
        # image tokens each) per sample, so a full batch of max_batch samples must fit one admission (otherwise decode would run
        # with a fraction of its rows filled)
        # spare KV slots (default: as many again as rows) let the scheduler prefill the next requests on a CU-masked stream while the
        # running rows decode (socioreasoner_amd/serving.py overlap); strategy_config overlap_admission: false = one stream as before
        self.overlap = bool(sc.get("overlap_admission", True))
        self.gen_stats = []          # one entry per generate call served by the scheduler (host preparation / run wall time, scheduler counters)
        kv_slots = int(sc.get("kv_slots", 2 * self.max_batch if self.overlap else 0))
        self.engine = Engine(self.geom, max_patches=int(sc.get("max_patches", self.max_batch * 2 * 2916)), kv_slots=kv_slots,
                             max_prefill_tokens=int(sc.get("max_prefill_tokens", min(prompt_len, 2048) * self.max_batch)),
                             max_batch=self.max_batch, max_ctx=max_ctx, max_new_tokens=min(resp_len, max_ctx - 1),
                             lm_fp8={"fp8": True, "fp8_e4m3": True, "fp8_mx": "mx"}.get(str(sc.get("quantization", "") or "").lower(), False),   # vLLM's knob name; fp8_mx: + MX fp8 activations in prefill
                             vit_fp8=_vision_quantization(sc),       # vision_quantization: fp8_mx -- the tower's own switch, not implied by `quantization`
                             device=f"cuda:{int(_get(getattr(self.worker, 'rank_info', None), 'local_rank', 0) or 0)}")
        if kind == "dir":
            self.engine.load_safetensors_dir(path)
            if any(os.path.exists(os.path.join(path, f)) for f in ("tokenizer.json", "tokenizer_config.json", "vocab.json")):
                from transformers import AutoTokenizer       # (a checkpoint with tokenizer files that do not load is an error, not a stub)
                self.tokenizer = AutoTokenizer.from_pretrained(path)
            else:
                logger.warning("checkpoint directory %r has no tokenizer files: token ids in, token ids out only", path)
                self.tokenizer = _StubTokenizer(self.geom)
        else:
            logger.warning("%s: using SYNTHETIC weights (seed %d)", path, int(sc.get("seed", 0)))
            self.engine.load_synthetic_weights(seed=int(sc.get("seed", 0)))
            self.tokenizer = _StubTokenizer(self.geom)
        self.command_queue = queue.Queue()
        ri = getattr(self.worker, "rank_info", None)
        if ri is not None:
            ri.dp_rank, ri.dp_size = getattr(self.worker, "rank", 0), getattr(self.worker, "world_size", 1)

    def load_states(self, *args, **kwargs):
        self._finish_weight_update()
        return None          # 7.5 GB of weights stay resident in 288 GB of HBM: nothing to reload

    def offload_states(self, include=None, non_blocking=False):
        return None

    # ------------------------------------------------------------------ trainer -> engine weight sync (reference
    # vllm_strategy.py:258-271 -> worker_helper.py:64-115).  The sender is rank `src_rank` of a torch.distributed group
    # (RCCL over xGMI on the node); with no group the update_* entry points can still be fed directly.
    def setup_collective_group(self, comm_plan, backend="nccl", rank_in_cluster=None):
        """Reference contract (strategy.py:85-113, third_party/vllm/worker_helper.py:68-92): find this worker in the comm plan,
        join the named group of its broadcast tree (RCCL over xGMI on the node; rank 0 = the trainer rank that owns the
        weights), warm the group up with one tiny all-reduce, remember the plan under its source pipeline rank."""
        import torch.distributed as dist
        from socioreasoner_amd.sync_group import join_named_group
        self.model_update_comm_plan = getattr(self, "model_update_comm_plan", {})
        me = int(getattr(self.worker, "rank", 0) or 0) if rank_in_cluster is None else int(rank_in_cluster)
        rank, args = hostops.get_dist_info_from_comm_plan(comm_plan, rank_in_cluster=me, rank_in_worker=0)
        if rank is None:
            logger.info("no comm_plan found for rank %s/0", me)
            return
        world = len(args["tgt_devices"]) + 1
        grp = join_named_group(args["group_name"], backend, world, rank, args["master_addr"], args["master_port"])
        # (the HIP current device is per THREAD: an RPC thread of a worker with local_rank > 0 would otherwise join the communicator on
        # device 0 -- bind everything of the weight-sync path to the ENGINE's device)
        edev = getattr(getattr(self, "engine", None), "device", None)
        if backend == "nccl" and edev is not None:
            torch.cuda.set_device(edev)
        dev = (edev if edev is not None else torch.device("cuda", torch.cuda.current_device())) if backend == "nccl" else torch.device("cpu")
        dist.all_reduce(torch.zeros(1, device=dev), group=grp)                 # warm-up, like the reference
        self.model_update_comm_plan[args["src_pp_rank"]] = dict(rank=rank, world_size=world, src_pp_rank=args["src_pp_rank"],
                                                                group_name=args["group_name"], comm_plan=comm_plan, comm_plan_args=args,
                                                                group=grp, device=dev)
        logger.info("joined %s as rank %d of %d", args["group_name"], rank, world)

    def _bcast(self, src_pp_rank, t: torch.Tensor):
        import torch.distributed as dist
        plan = getattr(self, "model_update_comm_plan", {}).get(src_pp_rank)
        if plan is None:
            return None                          # this engine rank is not a receiver of that pipeline stage (reference: silent no-op)
        xt = t.to(plan["device"])
        dist.broadcast(xt, src=0, group=plan["group"])
        return xt

    def _recv_device(self, src_pp_rank):
        plan = getattr(self, "model_update_comm_plan", {}).get(src_pp_rank)
        if plan is not None:
            if plan["device"].type == "cuda":
                torch.cuda.set_device(plan["device"])
            return plan["device"]
        edev = getattr(getattr(self, "engine", None), "device", None)
        return edev if edev is not None else ("cuda" if torch.cuda.is_available() else "cpu")

    def broadcast_bucket(self, src_pp_rank, meta_infos, bucket_size):
        dev = self._recv_device(src_pp_rank)
        buf = self._bcast(src_pp_rank, torch.empty(int(bucket_size), dtype=torch.int8, device=dev))
        if buf is not None:
            self.update_parameter_in_bucket(meta_infos, buf, [0])

    def broadcast_parameter(self, src_pp_rank, dtype, shape, parameter_name):
        dev = self._recv_device(src_pp_rank)
        w = self._bcast(src_pp_rank, torch.empty(tuple(shape), dtype=dtype, device=dev))
        if w is not None:
            self.update_parameter(parameter_name, w, [0])

    def update_parameter(self, parameter_name, weight, ranks_in_worker=None):
        self.engine.load_weight(parameter_name, weight)
        self._weights_dirty = True            # re-finalised (fp8: re-quantised) before the next generate

    def update_parameter_in_bucket(self, meta_infos, buffer, ranks_in_worker=None):
        from socioreasoner_amd.weight_sync import BucketReceiver
        if not hasattr(self, "_recv"):
            self._recv = BucketReceiver()
        for name, t in self._recv.process_bucket(meta_infos, buffer).items():
            self.update_parameter(name, t)

    def _finish_weight_update(self):
        if getattr(self, "_weights_dirty", False):
            if hasattr(self, "_recv"):
                self._recv.clear()
            self.engine.assert_ready()
            self._weights_dirty = False

    # ------------------------------------------------------------------ logits for callers that score sequences
    @torch.no_grad()
    def forward_step(self, batch: DataProto, forward_func) -> Dict[str, torch.Tensor]:
        """Reference contract (hf_strategy.py:49-94): micro-batches of (input_ids, attention_mask, position_ids [B,3,S],
        optional non_tensor_batch["multi_modal_inputs"] = per-sample {"pixel_values", "image_grid_thw"}); the model's
        logits [b, S, vocab] (bf16 like the HF forward; zeros at padded positions) go to
        forward_func(micro_batch, logits) -> (loss, dict), the dicts are collated."""
        from roll.datasets.collator import collate_fn_to_dict_list
        self._finish_weight_update()
        n = len(batch)
        mbs = int(batch.meta_info.get("micro_batch_size") or n)
        results = []
        for data in batch.chunk(max(n // max(mbs, 1), 1)):
            ids, mask, pos = data.batch["input_ids"], data.batch["attention_mask"].bool(), data.batch["position_ids"]
            if pos.dim() == 2:
                pos = pos[:, None, :].expand(-1, 3, -1)
            mm = data.non_tensor_batch.get("multi_modal_inputs") if data.non_tensor_batch else None
            b, S = ids.shape
            V = self.geom.text.vocab_size
            logits = torch.zeros(b, S, V, dtype=torch.bfloat16, device="cuda")
            i = 0
            while i < b:                               # groups bounded by the engine capacities
                grp, ntok = [], 0
                while i < b and len(grp) < self.max_batch:
                    k = int(mask[i].sum())
                    if grp and ntok + k > self.engine.cfg.max_prefill_tokens:
                        break
                    grp.append(i)
                    ntok += k
                    i += 1
                pix, grids = [], []
                for j in grp:
                    inp = mm[j] if mm is not None else None
                    if inp and "pixel_values" in inp:
                        pix.append(torch.as_tensor(inp["pixel_values"]).to("cuda", torch.float32))
                        grids += [tuple(int(v) for v in g_) for g_ in torch.as_tensor(inp["image_grid_thw"]).tolist()]
                emb = None
                if pix:
                    emb = self.engine.vit_forward(torch.cat(pix, dim=0).contiguous(), grids)     # HF processor layout [N, 1176] f32
                flat = self.engine.forward_logits([ids[j][mask[j]].cpu().numpy() for j in grp],
                                                  [pos[j][:, mask[j]].cpu().numpy() for j in grp], emb)
                o = 0
                for j in grp:
                    k = int(mask[j].sum())
                    logits[j, mask[j].to(logits.device)] = flat[o:o + k].to(torch.bfloat16)
                    o += k
            _, reduced = forward_func(data, logits.to(ids.device) if ids.device.type != "cuda" else logits)
            results.append(reduced)
        return collate_fn_to_dict_list(results)

    # ------------------------------------------------------------------ generate
    def _device_resize(self) -> bool:
        """strategy_config device_resize (default DEVICE_RESIZE_DEFAULT): a host image of a size the ViT cannot take is uploaded as it is and resized by
        sr_resize_pil_u8 (PIL's bicubic, bit for bit) instead of by PIL on the calling thread; false = the host resize."""
        v = self.__dict__.get("device_resize")
        if v is None:
            sc = _get(_get(getattr(self, "worker_config", None), "strategy_args"), "strategy_config", None) or {}
            v = self.device_resize = bool(dict(sc).get("device_resize", DEVICE_RESIZE_DEFAULT))
        return v

    def _prepare(self, ids: List[int], images, side_stream: bool = False) -> tuple:
        """-> (expanded ids np.int64, pos3 [3,S], list of uint8 HWC cuda images, grids).  side_stream: host images are uploaded on a stream of their
        own instead of the caller's current (usually the null) stream -- next to a running request loop a null-stream copy would wait for everything the
        scheduler's CU-masked streams have queued (they are blocking streams); the copy is synchronous for the host either way."""
        g = self.geom
        up = contextlib.nullcontext()
        if side_stream and torch.cuda.is_available():
            if getattr(self, "_upload_stream", None) is None:
                self._upload_stream = torch.cuda.Stream(self.engine.device if getattr(self, "engine", None) is not None else None)
            up = torch.cuda.stream(self._upload_stream)
        f = g.vision.patch_size * g.vision.spatial_merge_size
        ims, grids = [], []
        for im in images or []:
            if isinstance(im, torch.Tensor) and im.is_cuda:      # device-resident uint8 HWC (stage 2: the render kernel's output)
                h, w = int(im.shape[0]), int(im.shape[1])
                rh, rw = hostops.smart_resize(h, w, factor=f)
                if (rh, rw) == (h, w):
                    ims.append(im.contiguous())
                    grids.append((1, rh // g.vision.patch_size, rw // g.vision.patch_size))
                    continue
                if im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3:
                    # a size the ViT cannot take: PIL's bicubic resize as a kernel on the caller's stream, where the image lives (sr_resize_pil_u8;
                    # it replaces a copy to the host, the host resize and the upload, whatever device_resize says)
                    ims.append(raster.resize_pil(im, rh, rw, "bicubic"))
                    grids.append((1, rh // g.vision.patch_size, rw // g.vision.patch_size))
                    continue
                im = im.cpu().numpy()                            # (not uint8 RGB: bicubic resize on the host)
            arr = np.asarray(im.convert("RGB")) if hasattr(im, "convert") else np.asarray(im)
            h, w = arr.shape[:2]
            rh, rw = hostops.smart_resize(h, w, factor=f)
            on_device = (rh, rw) != (h, w) and self._device_resize() and arr.dtype == np.uint8 and arr.ndim == 3 and arr.shape[2] == 3
            if (rh, rw) != (h, w) and not on_device:
                from PIL import Image
                arr = np.asarray(Image.fromarray(arr).resize((rw, rh), resample=Image.BICUBIC))
            with up:
                t = torch.from_numpy(np.array(arr, dtype=np.uint8, order="C")).cuda()
                if on_device:
                    # uploaded at its own size, resized on the stream of the upload.  The pageable copy is synchronous for the host, the kernel is
                    # not: the image is handed on only after its stream has drained (a wait of microseconds), which is all the ordering the
                    # request loop has with the upload stream
                    t = raster.resize_pil(t, rh, rw, "bicubic")
                    torch.cuda.current_stream(t.device).synchronize()
                ims.append(t)
            grids.append((1, rh // g.vision.patch_size, rw // g.vision.patch_size))
        ids = np.asarray(ids, dtype=np.int64)
        n_pad = int((ids == g.image_token_id).sum())
        toks = [t * h * w // g.vision.spatial_merge_size ** 2 for t, h, w in grids]
        if grids and n_pad == len(grids):          # one placeholder per image (vLLM-style prompt): expand
            out, k = [], 0
            for t in ids.tolist():
                if t == g.image_token_id:
                    out += [t] * toks[k]
                    k += 1
                else:
                    out.append(t)
            ids = np.asarray(out, dtype=np.int64)
        elif grids and n_pad != sum(toks):
            raise ValueError(f"Image features and image tokens do not match: tokens: {n_pad}, features {sum(toks)}")
        pos3 = hostops.rope_index_1d(ids, grids or None, spatial_merge_size=g.vision.spatial_merge_size, image_token_id=g.image_token_id,
                                     vision_start_token_id=g.vision_start_token_id)      # (= get_rope_index of this one sequence, without torch's per-op cost)
        return ids, pos3, ims, grids

    @torch.no_grad()
    def generate(self, batch: DataProto, generation_config) -> torch.Tensor:
        self._finish_weight_update()
        gc = dict(generation_config)
        W = int(gc.get("num_beams", 1) or 1)
        if W > 1:
            check_beam_config(gc, self.engine.cfg.max_batch)
        lpn = check_logprobs_config(gc)
        greedy = sampling.is_greedy(gc) and float(gc.get("repetition_penalty", 1.0) or 1.0) == 1.0
        n = int(gc.get("num_return_sequences", 1) or 1)
        input_ids = batch.batch["input_ids"]
        attention_mask = batch.batch["attention_mask"]
        mm = batch.non_tensor_batch.get("multi_modal_data") if batch.non_tensor_batch else None
        prompts = hostops.gather_unpadded_input_ids(input_ids.cpu(), attention_mask.cpu())
        eos = gc.get("eos_token_id") or [self.tokenizer.eos_token_id]
        eos = [int(e) for e in (eos if isinstance(eos, (list, tuple)) else [eos])]
        pad = int(gc.get("pad_token_id", self.tokenizer.pad_token_id))
        max_new = min(int(gc["max_new_tokens"]), self.engine.cfg.max_new_tokens)
        B = len(prompts)
        results: List[List[List[int]]] = [None] * B          # per prompt: n responses
        prepared = []
        import time as _time
        t_gen0 = _time.perf_counter()
        for i in range(B):
            ids_i = mm[i]["prompt_token_ids"] if mm is not None and mm[i].get("prompt_token_ids") else prompts[i]
            imgs = (mm[i].get("multi_modal_data") or {}).get("image") if mm is not None else None
            prepared.append(self._prepare(ids_i, imgs))
        i = 0
        tk = gc.get("top_k", -1)
        # (round 5: top_k <= 0 / None = vLLM's "no top-k bound" is sampled on the device too -- k_sample_full, nucleus sampling over the whole vocabulary)
        tk = -1 if tk is None else int(tk)
        on_device = not greedy and tk <= 1024 and float(gc.get("temperature", 1.0)) > 1e-5
        rp1 = float(gc.get("repetition_penalty", 1.0) or 1.0) == 1.0
        if W > 1:
            self._generate_beam(prepared, results, gc, W, n, eos, pad, max_new)
            i = B
        elif greedy or on_device or sampling.is_greedy(gc):
            # the stages are decoupled: the scheduler admits the prompts in capacity-sized groups (ViT + prefill into free KV rows)
            # and ALL filled rows decode together -- a batch larger than one admission, or than max_batch, still decodes at full
            # width, and rows freed by short answers are refilled at once (socioreasoner_amd/serving.py).  Sampled n > 1: one request of n
            # sequences per prompt (chunks of at most max_batch), prefilled once and fanned out into n rows by the engine.  A repetition
            # penalty rides on the requests' own parameters (the per-row step); greedy with a penalty is the arg-max of the penalised logits
            from socioreasoner_amd.serving import ContinuousBatcher, Request
            g0 = sampling.is_greedy(gc)
            smp = None if g0 else {"temperature": float(gc.get("temperature", 1.0)), "top_k": int(tk), "top_p": float(gc.get("top_p", 1.0) or 1.0),
                                   "seed": int(gc.get("seed", 0) or 0) * 1000003 + 7919 * int(getattr(self.worker, "rank", 0) or 0)}
            own = None if rp1 else dict({k: v for k, v in (smp or {"temperature": 0.0}).items() if k != "seed"},
                                        repetition_penalty=float(gc.get("repetition_penalty", 1.0)))
            reqs, owner = [], []
            fan = 1 if g0 else n                       # greedy n > 1: the n answers are one answer, copied below
            mb = self.engine.cfg.max_batch
            for k in range(B):
                ids_k, pos_k, ims_k, grids_k = prepared[k]
                room = self.engine.cfg.max_ctx - len(ids_k)
                if room < 1:
                    raise ValueError(f"prompt of {len(ids_k)} tokens leaves no room in max_ctx {self.engine.cfg.max_ctx}")
                for c0 in range(0, fan, mb):
                    reqs.append(Request(ids=ids_k, pos3=pos_k, max_new=max(1, min(max_new, room)), images=ims_k, grids=grids_k, n=min(mb, fan - c0),
                                        sampling=own, logprobs=lpn))
                    owner.append(k)
            t_run0 = _time.perf_counter()
            cb = ContinuousBatcher(self.engine, eos, pad, sampling=smp, overlap=self.overlap)
            outs = cb.run(reqs)
            # where a generate call's wall time went (tools/run_example_small.py prints it): host preparation of the requests, then the scheduler's run
            self.gen_stats.append({"requests": B, "prepare_s": round(t_run0 - t_gen0, 3), "run_s": round(_time.perf_counter() - t_run0, 3),
                                   **{k: (round(v, 1) if isinstance(v, float) else v) for k, v in cb.stats.items()
                                      if k in ("admitted", "admitted_prompts", "steps", "steps_shared", "admissions", "rounds", "host_ms",
                                               "poll_wait_ms", "shares", "share_model")}})
            for k in range(B):
                results[k] = []
            recs = [[] for _ in range(B)]             # with logprobs: every response's records, cut like its tokens
            for k, r, out in zip(owner, reqs, outs):
                for j, row in enumerate(out if r.n > 1 else [out]):
                    row = [int(t) for t in row]
                    cut = next((j + 1 for j, t in enumerate(row) if t in eos), len(row))
                    results[k].append(row[:cut])
                    if lpn is not None:
                        rec = r.out_logprobs[j] if r.n > 1 else r.out_logprobs
                        recs[k].append((rec["logprobs"][:cut], rec["top"][:cut]))
            if g0:
                results = [rs * n for rs in results]
                recs = [rs * n for rs in recs]
            if lpn is not None:                        # one entry per row of the returned tensor, in its row order
                batch.meta_info["output_logprobs"] = [lp for rs in recs for lp, _ in rs]
                if lpn > 0:
                    batch.meta_info["output_top_logprobs"] = [top for rs in recs for _, top in rs]
            i = B
        while i < B:                                  # static batches (sampling with top-k above 1024)
            grp, ntok, npatch = [], 0, 0
            while i < B and len(grp) < self.max_batch:
                ids_i, _, _, grids = prepared[i]
                np_i = sum(t * h * w for t, h, w in grids)
                if grp and (ntok + len(ids_i) > self.engine.cfg.max_prefill_tokens or npatch + np_i > self.engine.cfg.max_patches):
                    break
                grp.append(i)
                ntok += len(ids_i)
                npatch += np_i
                i += 1
            ims = [im for k in grp for im in prepared[k][2]]
            grids = [g_ for k in grp for g_ in prepared[k][3]]
            emb = None
            if ims:
                pix = torch.cat([self.engine.patchify(im) for im in ims], dim=0)
                emb = self.engine.vit_forward(pix, grids)
            for k in grp:
                results[k] = []
            room = self.engine.cfg.max_ctx - max(len(prepared[k][0]) for k in grp)
            if room < 1:
                raise ValueError(f"prompt of {self.engine.cfg.max_ctx - room} tokens leaves no room in max_ctx {self.engine.cfg.max_ctx}")
            max_new_g = min(max_new, room)
            for rep in range(n):
                logits = self.engine.prefill([prepared[k][0] for k in grp], [prepared[k][1] for k in grp], emb, return_logits=not on_device)
                if on_device:          # k_sample inside the captured decode step
                    seed = int(gc.get("seed", 0) or 0) * 1000003 + 7919 * int(getattr(self.worker, "rank", 0) or 0) + 104729 * rep + grp[0]
                    toks = self.engine.decode_sample(max_new_g, float(gc.get("temperature", 1.0)), int(tk), float(gc.get("top_p", 1.0) or 1.0),
                                                     float(gc.get("repetition_penalty", 1.0) or 1.0), seed, eos=eos, pad_id=pad).cpu().tolist()
                else:
                    toks = self._sample_loop(logits, [prepared[k][0] for k in grp], max_new_g, eos, pad, gc).cpu().tolist()
                for row, k in zip(toks, grp):
                    cut = next((j + 1 for j, t in enumerate(row) if t in eos), len(row))
                    results[k].append(row[:cut])
        results = [r for rs in results for r in rs]
        output_ids = hostops.gather_outputs_to_pad_tensor(results, pad, device=input_ids.device)
        return hostops.concatenate_input_and_output(input_ids, output_ids, n)

    def _generate_beam(self, prepared, results, gc: dict, W: int, R: int, eos, pad: int, max_new: int):
        """num_beams W > 1 (HF _beam_search, do_sample=False): the prompts in chunks of max_batch // W (prompt tokens and image patches
        permitting), ViT and prefill once per chunk, then beam search on the device; results[k] gets prompt k's R hypotheses, best first,
        each cut after its eos."""
        lp = float(gc.get("length_penalty", 1.0) if gc.get("length_penalty") is not None else 1.0)
        per = max(1, self.engine.cfg.max_batch // W)
        B, i = len(prepared), 0
        while i < B:
            grp, ntok, npatch = [], 0, 0
            while i < B and len(grp) < per:
                ids_i, _, _, grids = prepared[i]
                np_i = sum(t * h * w for t, h, w in grids)
                if grp and (ntok + len(ids_i) > self.engine.cfg.max_prefill_tokens or npatch + np_i > self.engine.cfg.max_patches):
                    break
                grp.append(i)
                ntok += len(ids_i)
                npatch += np_i
                i += 1
            ims = [im for k in grp for im in prepared[k][2]]
            grids = [g_ for k in grp for g_ in prepared[k][3]]
            emb = None
            if ims:
                pix = torch.cat([self.engine.patchify(im) for im in ims], dim=0)
                emb = self.engine.vit_forward(pix, grids)
            room = self.engine.cfg.max_ctx - max(len(prepared[k][0]) for k in grp)
            if room < 1:
                raise ValueError(f"prompt of {self.engine.cfg.max_ctx - room} tokens leaves no room in max_ctx {self.engine.cfg.max_ctx}")
            self.engine.prefill([prepared[k][0] for k in grp], [prepared[k][1] for k in grp], emb)
            toks, _, lens = self.engine.decode_beam(W, min(max_new, room), R, lp, eos=eos, pad_id=pad)
            for g_, k in enumerate(grp):
                results[k] = [toks[g_, r, :int(lens[g_, r])].tolist() for r in range(R)]

    def _sample_loop(self, logits: torch.Tensor, prompt_ids, max_new: int, eos, pad: int, gc: dict) -> torch.Tensor:
        """Token-by-token decode with the draw on the host side of the C ABI (sr_decode_step).  -> int64 [B, max_new]"""
        B, V = logits.shape
        rp = float(gc.get("repetition_penalty", 1.0) or 1.0)
        seen = None
        if rp != 1.0:
            seen = torch.zeros(B, V, dtype=torch.bool, device=logits.device)
            for b, ids in enumerate(prompt_ids):
                seen[b, torch.as_tensor(np.asarray(ids), device=logits.device)] = True
        gen = getattr(self, "_generator", None)
        if gen is None:
            gen = self._generator = torch.Generator(device=logits.device)
            gen.manual_seed(int(gc.get("seed", 0) or 0) + 7919 * int(getattr(self.worker, "rank", 0) or 0))
        eos_t = torch.as_tensor(eos, device=logits.device)
        out = torch.full((B, max_new), pad, dtype=torch.int64, device=logits.device)
        done = torch.zeros(B, dtype=torch.bool, device=logits.device)
        for i in range(max_new):
            tok = sampling.sample(logits, float(gc.get("temperature", 1.0)), gc.get("top_k", -1), gc.get("top_p", 1.0), rp, seen, gen)
            tok = torch.where(done, torch.full_like(tok, pad), tok)
            out[:, i] = tok
            if seen is not None:
                seen[torch.arange(B, device=tok.device), tok] = True
            done |= torch.isin(tok, eos_t)
            if i + 1 == max_new or (i % 8 == 7 and bool(done.all())):
                break
            logits, _ = self.engine.decode_step(tok)
        return out

    # ------------------------------------------------------------------ request-level serving (generate_opt_level 1)
    def add_request(self, command, data: DataProto):
        if getattr(command, "name", command) == "ADD" and data is not None and data.batch is not None and getattr(self, "engine", None) is not None:
            # the host side of a request (image resize + upload, placeholder expansion, rope index: ~1 ms) is done HERE, on the caller's thread, not
            # between two scheduling rounds of the request loop
            try:
                mm = data.non_tensor_batch.get("multi_modal_data") if data.non_tensor_batch else None
                ids_in = hostops.gather_unpadded_input_ids(data.batch["input_ids"].cpu(), data.batch["attention_mask"].cpu())[0]
                if mm is not None and mm[0].get("prompt_token_ids"):
                    ids_in = mm[0]["prompt_token_ids"]
                imgs = (mm[0].get("multi_modal_data") or {}).get("image") if mm is not None else None
                data.meta_info["_prepared"] = self._prepare(ids_in, imgs, side_stream=True)
            except Exception as e:  # noqa: BLE001  (the request loop prepares it again and raises where the reference's loop would)
                data.meta_info.pop("_prepared", None)
                logger.debug("request preparation deferred to the request loop: %s", e)
        self.command_queue.put((command, data))

    def start_server(self, data: DataProto, request_complete_callback):
        """Request-level serving (reference vllm_strategy.py:156-205): ADD / ABORT / STOP commands arrive through the queue
        while the loop runs; greedy requests and sampling requests with a top-k bound of at most 1024 (any repetition penalty) are served by
        CONTINUOUS batching (socioreasoner_amd.serving: admit on finish, one graph replay per token for all rows, the draw inside the graph; a
        sampled request with num_return_sequences n > 1 is admitted once and fanned out into n rows).  The batcher's shared configuration is
        that of the request that opened it; a request with other sampling parameters, or a repetition penalty, joins the running rows under
        its own parameters (Request.sampling: its seed gives the streams (seed, fork); without a seed the batcher derives one per request, so
        two such requests with the same prompt draw differently).  Static batches, after the running rows have drained, remain for: an eos
        set or pad id other than the running batcher's, num_beams > 1, a top-k bound above 1024 and n above the engine's rows.  Each request
        is reported through the callback the moment its last sequence ends, with its n token lists in output_token_ids."""
        from socioreasoner_amd.serving import ContinuousBatcher, Request
        self.running = True
        batcher, bkey, bdkey = None, None, None
        sampled: List[DataProto] = []
        stop = False
        last_cmd = 0.0
        while True:
            busy = batcher is not None and not batcher.idle()
            try:
                command, req = self.command_queue.get(timeout=0.0005 if busy or sampled else 0.01)
            except queue.Empty:
                command, req = None, None
            # every queued command is taken before the next scheduling round: at one command per round a burst of ADDs -- the two-stage pipeline's
            # stage-2 prompts of a wave that has just finished -- would trickle into the scheduler one request per steps_per_poll decode steps
            taken = 0
            while command is not None or taken == 0:
                taken += 1
                name = getattr(command, "name", command)
                if name == "ADD":
                    gc = dict(req.meta_info.get("generation_config") or {})
                    greedy = sampling.is_greedy(gc)
                    tk = gc.get("top_k", -1)
                    tk = -1 if tk is None else int(tk)
                    dev_sampling = not greedy and tk <= 1024 and float(gc.get("temperature", 1.0)) > 1e-5
                    n_req = int(gc.get("num_return_sequences", 1) or 1)
                    rp = float(gc.get("repetition_penalty", 1.0) or 1.0)
                    lpn = check_logprobs_config(gc)
                    rows_ok = (hasattr(self.engine, "rows_begin") and (greedy or dev_sampling) and rp > 0
                               and n_req <= getattr(getattr(self.engine, "cfg", None), "max_batch", 1)
                               and int(gc.get("num_beams", 1) or 1) == 1)          # beam search: the static path (generate's beam branch)
                    if not rows_ok:
                        sampled.append(req)
                    else:
                        eos = gc.get("eos_token_id") or [self.tokenizer.eos_token_id]
                        eos = [int(e) for e in (eos if isinstance(eos, (list, tuple)) else [eos])]
                        pad = int(gc.get("pad_token_id", self.tokenizer.pad_token_id))
                        base_seed = int(gc.get("seed", 0) or 0) * 1000003 + 7919 * int(getattr(self.worker, "rank", 0) or 0)      # (as generate())
                        smp = None if greedy else {"temperature": float(gc.get("temperature", 1.0)), "top_k": int(tk),
                                                   "top_p": float(gc.get("top_p", 1.0) or 1.0), "seed": base_seed}
                        key = (tuple(eos), pad)
                        dkey = None if smp is None else tuple(sorted(smp.items()))
                        # a new batcher (its shared configuration = this request's) only when none runs; a running one takes requests with other
                        # sampling parameters into its rows, each under its own parameters (the per-row step)
                        if batcher is None or (batcher.idle() and (key, dkey) != (bkey, bdkey)):
                            if batcher is not None:
                                batcher._hand_back()      # (the engine's log-prob recording off again before the batcher goes)
                            batcher, bkey, bdkey = ContinuousBatcher(self.engine, eos, pad, sampling=smp, overlap=self.overlap), key, dkey
                        if key != bkey:
                            sampled.append(req)          # a different stop set / pad id while rows are running: static path
                        else:
                            own = None
                            if dkey != bdkey or rp != 1.0:
                                own = {"temperature": 0.0 if greedy else float(gc.get("temperature", 1.0)), "top_k": int(tk),
                                       "top_p": float(gc.get("top_p", 1.0) or 1.0), "repetition_penalty": rp}
                                if gc.get("seed") is not None:      # its own seed: streams (seed, fork); without one the batcher derives a seed per request
                                    own["seed"] = base_seed
                            if req.meta_info.get("_prepared") is not None:          # done by add_request on the caller's thread
                                ids, pos3, ims, grids = req.meta_info.pop("_prepared")
                            else:
                                mm = req.non_tensor_batch.get("multi_modal_data") if req.non_tensor_batch else None
                                ids_in = hostops.gather_unpadded_input_ids(req.batch["input_ids"].cpu(), req.batch["attention_mask"].cpu())[0]
                                if mm is not None and mm[0].get("prompt_token_ids"):
                                    ids_in = mm[0]["prompt_token_ids"]
                                imgs = (mm[0].get("multi_modal_data") or {}).get("image") if mm is not None else None
                                ids, pos3, ims, grids = self._prepare(ids_in, imgs)
                            room = self.engine.cfg.max_ctx - len(ids)
                            if room < 1:
                                raise ValueError(f"prompt of {len(ids)} tokens leaves no room in max_ctx {self.engine.cfg.max_ctx}")
                            max_new = max(1, min(int(gc["max_new_tokens"]), self.engine.cfg.max_new_tokens, room))
                            batcher.submit(Request(ids=ids, pos3=pos3, max_new=max_new, images=ims, grids=grids, tag=req,
                                                   n=1 if greedy else n_req, sampling=own, logprobs=lpn))          # (greedy: the n answers are one answer)
                elif name == "ABORT":
                    rid = req.meta_info["request_id"]
                    sampled = [p for p in sampled if p.meta_info.get("request_id") != rid]
                    if batcher is not None:      # queued requests are dropped, running rows stop now and free row + KV slot at the next poll
                        batcher.abort(lambda r: r.tag.meta_info.get("request_id") == rid)
                elif name == "STOP":
                    stop = True
                if command is None or taken >= 1024:
                    break
                try:
                    command, req = self.command_queue.get_nowait()
                except queue.Empty:
                    break
            if taken > 1 or command is not None:
                last_cmd = time.monotonic()
            # with no rows running, a first admission of a few requests would leave the rest of a burst that is still arriving (one ADD per ~1 ms of the
            # producer's preparation) waiting for a whole admission: the loop waits until a full group is pending or nothing has arrived for 5 ms
            filling = (batcher is not None and not batcher.active and batcher.staged is None and 0 < len(batcher.pending) < self.max_batch
                       and not stop and time.monotonic() - last_cmd < 0.005)
            if batcher is not None and not batcher.idle() and not filling and (self.command_queue.empty() or len(batcher.active) > 0):
                def done(r, toks):
                    if r.aborted:
                        return
                    res = DataProto(meta_info=dict(r.tag.meta_info))
                    n_out = int((r.tag.meta_info.get("generation_config") or {}).get("num_return_sequences", 1) or 1)
                    lists = toks if r.n > 1 else [toks] * n_out
                    res.meta_info["output_token_ids"] = [[int(t) for t in x] for x in lists]
                    if r.logprobs is not None:      # next to the tokens, one entry per token list
                        recs = r.out_logprobs if r.n > 1 else [r.out_logprobs] * n_out
                        res.meta_info["output_logprobs"] = [list(x["logprobs"]) for x in recs]
                        if r.logprobs > 0:
                            res.meta_info["output_top_logprobs"] = [list(x["top"]) for x in recs]
                    request_complete_callback(data=res)
                batcher.pump(done)
            if sampled and (len(sampled) >= self.max_batch or self.command_queue.empty()):
                todo, sampled = sampled[: self.max_batch], sampled[self.max_batch:]
                gc = todo[0].meta_info.get("generation_config")
                if int((gc or {}).get("num_beams", 1) or 1) > 1:     # beam requests are served only with their own generation config
                    same = [r for r in todo if r.meta_info.get("generation_config") == gc]
                    sampled = [r for r in todo if r.meta_info.get("generation_config") != gc] + sampled
                    todo = same
                # one generate call runs under ONE config: requests that ask for other log-probs (or none) than the first wait for a batch of their own
                lp_of = lambda r: (r.meta_info.get("generation_config") or {}).get("logprobs")
                sampled = [r for r in todo if lp_of(r) != lp_of(todo[0])] + sampled
                todo = [r for r in todo if lp_of(r) == lp_of(todo[0])]
                if batcher is not None and not batcher.idle():
                    sampled = todo + sampled      # rows are running: the static path needs the whole engine, wait
                else:
                    merged = DataProto.concat(todo)
                    if batcher is not None:
                        batcher._hand_back()          # (the engine's log-prob recording off again before the batcher goes)
                    out = self.generate(merged, gc)
                    batcher = None                # generate() re-initialises the batch rows
                    P = merged.batch["input_ids"].shape[1]
                    n_out = int(gc.get("num_return_sequences", 1) or 1)
                    for i_r, r in enumerate(todo):         # n rows per request, adjacent
                        res = DataProto(meta_info=dict(r.meta_info))
                        res.meta_info["output_token_ids"] = [[int(t) for t in row[P:].tolist() if int(t) != int(gc.get("pad_token_id", -1))]
                                                             for row in out[i_r * n_out:(i_r + 1) * n_out]]
                        for key in ("output_logprobs", "output_top_logprobs"):      # generate() recorded them per row of `out`
                            if key in merged.meta_info:
                                res.meta_info[key] = merged.meta_info[key][i_r * n_out:(i_r + 1) * n_out]
                        request_complete_callback(data=res)
            if stop and (batcher is None or batcher.idle()) and not sampled:
                self.running = False
                if batcher is not None:
                    batcher._hand_back()
                if batcher is not None and hasattr(self, "gen_stats"):      # (as generate(): what the scheduler did while this server was open)
                    self.gen_stats.append({"requests": batcher.stats["admitted"], "served_as": "request stream",
                                           **{k: (round(v, 1) if isinstance(v, float) else v) for k, v in batcher.stats.items()
                                              if k in ("steps", "steps_shared", "admissions", "rounds", "host_ms", "poll_wait_ms", "shares", "share_model")}})
                return


def check_logprobs_config(gc: dict):
    """generation_config["logprobs"]: absent / None = off (-> None), N in 0..8 = the log-prob of every response token under the raw logits and
    the N most likely tokens of its step (vLLM's SamplingParams.logprobs; the engine records them in the step that picks the token).  What
    the engine does not record is refused by name."""
    lp = gc.get("logprobs")
    if lp is None:
        return None
    if isinstance(lp, bool) or int(lp) != lp or not 0 <= int(lp) <= 8:
        raise ValueError(f"logprobs={lp!r} is outside the engine's range 0..8 (top-N entries per token)")
    W = int(gc.get("num_beams", 1) or 1)
    if W > 1:
        raise NotImplementedError(f"logprobs={lp} together with num_beams={W} is not supported (beam search returns summed log-probs as its scores)")
    tk = gc.get("top_k", -1)
    tk = -1 if tk is None else int(tk)
    if tk > 1024 and not sampling.is_greedy(gc):
        raise NotImplementedError(f"logprobs={lp} together with top_k={tk} > 1024 is not supported (that draw runs on the host, outside the "
                                  "step that records log-probs)")
    return int(lp)


def check_beam_config(gc: dict, max_batch: int):
    """The beam-search settings generate() serves (HF _beam_search with do_sample=False, early_stopping=False); the rest is refused by name."""
    W = int(gc.get("num_beams", 1) or 1)
    R = int(gc.get("num_return_sequences", 1) or 1)
    if not 1 <= R <= W:
        raise ValueError(f"num_return_sequences={R} must be between 1 and num_beams={W}")
    if W > min(8, max_batch):
        raise ValueError(f"num_beams={W} exceeds the engine's limit of {min(8, max_batch)} beams per prompt")
    if float(gc.get("repetition_penalty", 1.0) or 1.0) != 1.0:
        raise NotImplementedError(f"repetition_penalty={gc.get('repetition_penalty')} together with num_beams={W} is not supported")
    es = gc.get("early_stopping", False)
    if es is True or es == "never":
        raise NotImplementedError(f"early_stopping={es!r} together with num_beams={W} is not supported (only early_stopping=False)")


class SegRasterStrategy(InferenceStrategy):
    """SegInferStrategy.segment (seg_strategy.py:26-72): 756 x 756 resize, ``set_image``, per object predict -> arg-max score -> OR, nearest
    756 -> 768.  ``model_provider`` returns the predictor: roll.models.model_providers.sam2_seg_model_provider gives the MI355X SAM2
    (socioreasoner_amd.sam2.Sam2Predictor: the whole object loop on the device); any object with set_image(image) /
    predict(**prompt) -> (masks, scores, _) works through the generic loop below."""
    strategy_name = "seg_infer"

    def initialize(self, model_provider=None):
        self.model = model_provider(model_args=_get(self.worker_config, "model_args"), is_trainable=False) if model_provider else None

    def load_states(self, *args, **kwargs):
        return None

    def offload_states(self, *args, **kwargs):
        return None

    def _resized(self, image):
        """image.resize((756, 756)) (seg_strategy.py:44), remembered per image OBJECT: the second stage segments the image the first stage did
        (3.7 ms of PIL bicubic per call).  The host path: with strategy_config device_resize on and a predictor that takes
        ``resize_to`` the original images go to the device and neither this method nor its memo is used (`_resize_on_device`)."""
        from collections import OrderedDict
        import threading
        memo = self.__dict__.setdefault("_r756", OrderedDict())
        lock = self.__dict__.setdefault("_r756_lock", threading.Lock())      # (the prefetch thread resizes too)
        with lock:
            hit = memo.get(id(image))
            if hit is not None and hit[0] is image:
                memo.move_to_end(id(image))
                return hit[1]
        r = image.resize((756, 756))
        with lock:
            memo[id(image)] = (image, r)
            while len(memo) > 1024:
                memo.popitem(last=False)
        return r

    _device_resize = Mi355xStrategy._device_resize      # strategy_config device_resize

    def _resize_on_device(self, images) -> bool:
        """True when the predictor resizes on the device (socioreasoner_amd.sam2.Sam2Predictor: ``resize_to``) and the switch is on: the ORIGINAL
        images go in, neither `_resized` nor its memo is used.  Images that are not plain RGB (PIL converts after the resize there, the device path
        before it) keep the host path."""
        import inspect
        fn = getattr(self.model, "segment_batch", None)
        if fn is None or not self._device_resize():
            return False
        try:
            if "resize_to" not in inspect.signature(fn).parameters:
                return False
        except (TypeError, ValueError):
            return False
        return all(getattr(im, "mode", "RGB") == "RGB" and (hasattr(im, "mode") or (getattr(im, "ndim", 0) == 3 and im.shape[2] == 3 and str(im.dtype).endswith("uint8")))
                   for im in images)

    def prefetch(self, images, chunk=None) -> None:
        """Round 6: start SAM2's image encoder on these images in the background (socioreasoner_amd.sam2.Sam2Predictor.prefetch); `segment` later finds
        the embeddings cached.  Predictors without `prefetch` (the reference's SAM2ImagePredictor) ignore the hint."""
        if self.model is not None and hasattr(self.model, "prefetch"):
            images = list(images)
            if self._resize_on_device(images):
                self.model.prefetch(images, chunk=chunk, resize_to=(756, 756))      # (the 756 x 756 resize is a kernel on the upload stream)
                return
            self.model.prefetch(images, prepare=self._resized, chunk=chunk)      # (the 756 x 756 resize, 3.7 ms per image, on the prefetch thread as well)

    def wait_prefetch(self) -> None:
        if self.model is not None and hasattr(self.model, "wait_prefetch"):
            self.model.wait_prefetch()

    def segment(self, batch: DataProto) -> dict:
        images, prompts = list(batch.non_tensor_batch["seg_image"]), list(batch.non_tensor_batch["visual_prompt"])
        masks: list = [None] * len(images)
        live = [i for i, vp in enumerate(prompts) if len(vp) > 0]
        for i in range(len(images)):
            if i not in live:
                masks[i] = np.zeros((768, 768), dtype=np.uint8)       # seg_strategy.py:36-38: nothing to segment
        if live and self.model is None:
            raise RuntimeError("seg_infer needs a SAM2-compatible predictor (not available offline)")
        if live and hasattr(self.model, "segment_batch"):
            # socioreasoner_amd.sam2: the encoder runs over several images per pass (and not at all for an image it has seen: stage 2
            # segments stage 1's image), decode / arg-max / resize / threshold / OR stay on the device
            if self._resize_on_device([images[i] for i in live]):
                accs = self.model.segment_batch([images[i] for i in live], [prompts[i] for i in live], resize_to=(756, 756))
            else:
                accs = self.model.segment_batch([self._resized(images[i]) for i in live], [prompts[i] for i in live])
            for i, acc in zip(live, accs):
                masks[i] = raster.resize_nearest(acc, 768, 768).cpu().numpy()
            live = []
        for i in live:
            image, visual_prompt = images[i], prompts[i]
            self.model.set_image(image.resize((756, 756)))
            dev = getattr(getattr(self.model, "engine", None), "device", None) or torch.device("cuda", torch.cuda.current_device())
            acc = torch.zeros(756, 756, dtype=torch.uint8, device=dev)
            for vp in visual_prompt:
                try:
                    prompt = {k: vp[k] for k in ("point_coords", "point_labels", "box") if k in vp}
                    pred_masks, scores, _ = self.model.predict(**prompt)
                    best = np.ascontiguousarray(np.asarray(pred_masks[int(np.argmax(scores))]).astype(np.uint8))
                    raster.mask_union_(acc, torch.from_numpy(best).to(dev))
                except Exception:  # noqa: BLE001  (the reference swallows per-object failures, seg_strategy.py:61-62)
                    continue
            masks[i] = raster.resize_nearest(acc, 768, 768).cpu().numpy()
        out = np.empty(len(masks), dtype=object)
        for i, m in enumerate(masks):
            out[i] = m
        return {"mask": out}
