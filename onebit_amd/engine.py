"""Fused whole-token greedy decode (batch 1) -- SURVEY.md section 8(f) rank 1.

``DecodeEngine`` drives ``onebit_decode_step`` (include/onebit.h): 5 HIP launches per decoder
layer + lm_head + argmax, every 1-bit projection read once in the reference's packed layout,
LayerNorm / RMSNorm / RoPE / SiLU / residuals fused into the consumers' prologues, token id and
position kept on the device.  One decode step is captured into a HIP graph (via
``torch.cuda.CUDAGraph``) and replayed per token -- 160+ launches per token would otherwise be
host-bound (the reference issues ~10 ATen launches per BitLinearInf call).

Prefill of the prompt (S > 1) runs through the module path (``OneBitLlamaForCausalLM.forward``)
into the same preallocated KV cache.
"""
from __future__ import annotations

import copy
import ctypes
from typing import List, Optional

import torch

from . import _lib
from ._abi import (KSEG_ATTN_O, KSEG_DOWN, KSEG_GATE_UP, KSEG_HEAD, KSEG_QKV, PRO_EMBED_RMS, PRO_PLAIN, PRO_RES_LN_RMS,  # noqa: F401
                   PRO_SWIGLU, _BatchState, _FusedIn, _KState, _Layer, _MixedState, _Model, _Proj, _Seg, _SpecState, _State,
                   _model_struct, _proj, _vp, make_state, tile_stats_floats)
from .llama import KVCache, OneBitLlamaForCausalLM, _cut_at_eos


def _check_params(params: torch.Tensor, rows: int, dev) -> None:
    """Device rows of onebit_sample_params_t for a sampled step (sampling.pack)."""
    if params.dtype != torch.uint8 or params.dim() != 2 or params.shape[0] < rows or params.shape[1] != 32 or \
            not params.is_contiguous() or params.device != dev:
        raise ValueError(f"sampling params must be contiguous uint8 [>= {rows}, 32] on {dev} (onebit_amd.sampling.pack)")


def _call(lib, dev, name: str, *args) -> None:
    """``lib.<name>(*args, stream)`` on ``dev``'s current stream; a non-zero return code raises (``_lib.check``)."""
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(*args, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, name)


def _capture(fn) -> torch.cuda.CUDAGraph:
    """A HIP graph of ``fn()`` on the capture stream."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def _argmax_parts(vocab: int, dev):
    """(part_val, part_idx): the lm_head argmax partials of the batched, mixed and speculative steps."""
    n = -(-vocab // 128) * 64
    return torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)


def _aligned_ws(nbytes: int, dev):
    """(tensor, offset): a zeroed workspace of ``nbytes`` bytes from the 256-byte aligned address ``data_ptr() + offset``."""
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=dev)
    return ws, (-ws.data_ptr()) % 256


def _bind(model: OneBitLlamaForCausalLM, caches, n_slots: int, max_len: int, who: str):
    """What every step class starts with: the model on a GPU and in fp16 (``fp16_view``), ``max_len`` inside the rope tables,
    ``caches[l] = (k, v)`` contiguous fp16 ``[n_slots, n_kv_heads, max_len, head_dim]`` on the model's device.  Returns
    (fp16 model, config, device, library, ``onebit_model_t`` image, objects that must outlive the image)."""
    if not model.lm_head.weight.is_cuda:
        raise RuntimeError(f"{who} needs the model on a ROCm GPU (no CPU fallback)")
    model = fp16_view(model)        # an fp32 checkpoint: floating parameters cast once, packed weights shared
    cfg, dev = model.config, model.lm_head.weight.device
    if max_len > cfg.max_position_embeddings:
        raise ValueError("max_len exceeds max_position_embeddings (the rope tables have that many rows)")
    shape = (n_slots, cfg.num_key_value_heads, max_len, cfg.head_dim)
    for i, (kc, vc) in enumerate(caches):
        if tuple(kc.shape) != shape or tuple(vc.shape) != shape or not kc.is_contiguous() or not vc.is_contiguous():
            raise ValueError(f"cache {i} must be contiguous {shape}")
        # the attention kernels read and write the caches as fp16 on the model's device whatever the checkpoint's
        # dtype: an fp32 model's own new_cache() would be reinterpreted silently (results wrong, nothing out of bounds)
        if kc.dtype != torch.float16 or vc.dtype != torch.float16:
            raise ValueError(f"cache {i} must be float16 (got {kc.dtype} / {vc.dtype}): build the caches with "
                             f"fp16_view(model).new_cache({n_slots}, {max_len})")
        if kc.device != dev or vc.device != dev:
            raise ValueError(f"cache {i} must be on the model's device {dev}")
    struct, keep = _model_struct(model, caches, max_len)
    return model, cfg, dev, _lib.load(), struct, keep


def step_variant(steps: int, long_from: int, short_ok: bool, keyblock: bool, kb_chunk: int, kb_top: int):
    """Which form of ``onebit_decode_step`` serves the step that follows ``steps`` cached tokens (the key of
    ``DecodeEngine._variants``).  The split-KV forms take over from ``long_from`` (0: never), or everywhere when the
    one-workgroup form's scores do not fit its LDS (``short_ok`` False): key-block attention as ``("kb", ns)``, ``ns`` the smallest
    power of two with ``ns * kb_chunk >= steps + 1`` (the step attends to positions 0 .. steps) up to ``kb_top``, the largest
    split count built, or the scores + P.V pair ``"long"``.  Below that ``"64"`` while the position is under 64 (``attn_blind``), else ``"short"``."""
    if bool(long_from) and (steps >= long_from or not short_ok):
        if not keyblock:
            return "long"
        ns = 1
        while ns * kb_chunk < steps + 1 and ns < kb_top:
            ns *= 2
        return ("kb", ns)
    return "64" if steps < 64 else "short"


def fused_gemv(mods, outs, prologue, rms_eps=1e-6, ln_eps=1e-5, stats_out=None, **inputs):
    """One ``onebit_fused_gemv`` launch on the current stream: projections ``mods`` (BitLinearInf
    sharing in_features) write their pre-LayerNorm outputs to ``outs`` (fp16 [N_i] tensors);
    ``inputs`` are the prologue tensors named as in ``onebit_fused_in_t`` (``st_prev`` / ``st_gate``
    / ``st_up``: tile partials of the corresponding vectors, fp32 ``tile_stats_floats(n)``);
    ``stats_out[i]``: where projection i publishes its own partials (or None)."""
    n = len(mods)
    projs = (_Proj * n)(*[_proj(m) for m in mods])
    optr = (_vp * n)(*[o.data_ptr() for o in outs])
    so = list(stats_out or []) + [None] * 3
    st_out = (_vp * 3)(*[t.data_ptr() if t is not None else None for t in so[:3]])
    fin = make_state(_FusedIn, inputs, rms_eps=rms_eps, ln_eps=ln_eps, st_out=st_out)
    _call(_lib.load(), outs[0].device, "onebit_fused_gemv", ctypes.cast(projs, _vp), ctypes.cast(optr, _vp), n, prologue, ctypes.byref(fin))


def fp16_view(model: OneBitLlamaForCausalLM) -> OneBitLlamaForCausalLM:
    """The model the fused engines run: every floating parameter in fp16, the packed int8 weights SHARED with
    ``model`` (not copied).  An fp16 model is returned as is.  This is what the reference's
    ``from_pretrained(..., torch_dtype=torch.float16)`` does to the released FP32 checkpoints
    (/root/reference/checkpoints/README.md:10; modeling_utils.py:696 casts floating parameters only), done once
    at engine build instead of making the caller find out; the caller's fp32 model is left untouched."""
    if all(p.dtype == torch.float16 for p in model.parameters() if p.is_floating_point()):
        return model
    memo = {id(p): p for p in model.parameters() if not p.is_floating_point()}
    return copy.deepcopy(model, memo).half()


class DecodeEngine:
    def __init__(self, model: OneBitLlamaForCausalLM, max_len: int, use_graph: bool = True,
                 long_context_from: int = 160, attn_splits: int = 8, long_attention: str = "keyblock", attn_chunk: int = 128,
                 native_prefill: bool = True, prefill_rows: int = 2048):
        """``native_prefill``: ``generate`` / ``prime`` run the prompt through ``onebit_mixed_step`` (one C call per ``prefill_rows``
        prompt tokens, lm_head on the last row only) instead of the module path -- time to first token on 7B shapes 16.5 -> 2.3 ms at 16
        prompt tokens, 19.7 -> 5.3 at 128, 23.5 -> 12.2 at 512, 66 -> 24.5 at 2040 (tools/ttft_probe.py).  ``prefill`` keeps the module
        path: it returns the logits of every prompt row.
        ``long_context_from``: position from which a step uses a split-KV attention graph; below it one workgroup per head
        with the first 128 positions' scores in registers is faster (measured crossover on 7B: 0.947 vs 0.963 ms / token at 132-164
        cached tokens, 1.184 vs 0.971 at 260-292: tools/ctx_probe.py).  0 disables.
        ``long_attention``: "keyblock" (round 6, default: LayerNorm + RoPE + cache append in one launch, then
        ``onebit_attention_decode_rows`` -- ``attn_chunk`` positions per workgroup, K and V read once, last-arriver combine; one
        HIP graph per power-of-two split count, chosen per step by the host-known position) or "pair" (round 2: scores kernel +
        P.V kernel with ``attn_splits`` splits, the reference's fp16 probability rounding)."""
        if long_attention not in ("keyblock", "pair"):
            raise ValueError("long_attention must be 'keyblock' or 'pair'")
        self.max_len = int(max_len)
        cfg, dev, f16 = model.config, model.lm_head.weight.device, torch.float16
        if self.max_len > cfg.max_position_embeddings:                      # (before the cache below is allocated)
            raise ValueError("max_len exceeds max_position_embeddings")
        self.cache = KVCache(cfg, 1, self.max_len, dev, f16)
        self.model, self.cfg, self.dev, self.lib, self._model, self._keep = _bind(model, self.cache.layers, 1, self.max_len, "DecodeEngine")
        H, I, D = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
        self._native_prefill, self._prefill_rows, self._mixed = bool(native_prefill), max(int(prefill_rows), 64), None
        z = lambda n, dt=f16: torch.zeros(n, dtype=dt, device=dev)
        self.token = z(1, torch.int32)
        self.pos = z(1, torch.int32)
        self.out_tokens = z(self.max_len, torch.int32)
        Hq, Hkv = cfg.num_attention_heads * D, cfg.num_key_value_heads * D
        self.buf = dict(hres0=z(H), hres1=z(H), u_q=z(Hq), u_k=z(Hkv), u_v=z(Hkv), attn_out=z(Hq), u_o=z(H),
                        u_gate=z(I), u_up=z(I), u_down=z(H), logits=z(cfg.vocab_size),
                        part_val=z(1024, torch.float32), part_idx=z(1024, torch.int32))
        self._rope_cur = z(2 * D)
        self._tile_stats = z(max(int(self.lib.onebit_decode_stats_floats(ctypes.byref(self._model))), 1), torch.float32)
        # sampled decoding: the armed request's onebit_sample_params_t row (device: the graphs read it at replay); the sampled
        # graphs are captured on first use next to the greedy ones (which stay as they are)
        self._params = torch.zeros(1, 32, dtype=torch.uint8, device=dev)
        self._sampled = False
        self._use_graph = bool(use_graph)
        self._spec_steps = {}               # (draft_tokens, ngram_max, ngram_min) -> SpecStep
        self._prompt_len = 0
        self._steps = 0                     # host-side count of tokens in the cache (chooses the variant)
        self._long_from = int(long_context_from) if long_context_from and self.max_len > long_context_from else 0
        # the one-workgroup-per-head attention keeps the scores of every position in LDS (64 KiB limit
        # in onebit_decode_step): beyond that only the split-KV form exists, and it serves every position
        self._short_ok = 512 + 3 * 128 * 2 + 8 * 128 * 4 + 4 * self.max_len <= 64 * 1024
        if not self._short_ok:
            if not long_context_from:
                raise ValueError(f"max_len {self.max_len} needs the split-KV attention (long_context_from > 0)")
            self._long_from = 1
        # The forms of the step (``step_variant`` picks one per step by the host-known position): one state each, and one HIP graph
        # per (form, sampled).  "64" -- steps at positions < 64: the attention requests half the rows before it knows the position
        # (onebit.h, attn_blind); the same arithmetic.
        short = make_state(_State, dict(self.buf, token=self.token, pos=self.pos, out_tokens=self.out_tokens, rope_cur=self._rope_cur,
                                        tile_stats=self._tile_stats), max_out=self.max_len)
        self._variants = {"short": short, "64": make_state(short, attn_blind=64)}
        self._graphs = {}
        if self._short_ok:
            self._warm("short")
            self._warm("64")
        self._keyblock = long_attention == "keyblock" and bool(self._long_from)
        self._kb_chunk = self._kb_top = 0
        self._scratch = []
        if self._keyblock:
            # one state / graph per power-of-two split count: splits * attn_chunk covers the step's context + 1
            if attn_chunk < 64 or attn_chunk % 64:
                raise ValueError("attn_chunk must be a positive multiple of 64")
            self._kb_chunk = int(attn_chunk)
            top = -(-self.max_len // self._kb_chunk)
            if top > 64:
                self._kb_chunk = 64 * -(-self.max_len // (64 * 64))          # at most 64 splits: widen the chunk
                top = -(-self.max_len // self._kb_chunk)
            self._q_rows = z(Hq)
            ns = 1
            while True:
                nb = int(self.lib.onebit_attention_decode_scratch_bytes(1, cfg.num_attention_heads, ns))
                self._scratch.append(z(max(nb, 16), torch.uint8))
                self._variants[("kb", ns)] = make_state(short, dict(q_rows=self._q_rows, attn_scratch=self._scratch[-1]),
                                                        attn_splits=ns, attn_chunk=self._kb_chunk)
                self._kb_top = ns
                self.pos.zero_()
                self._warm(("kb", ns))
                if ns >= top:
                    break
                ns *= 2
        elif self._long_from:
            S = max(2, min(int(attn_splits), 16, self.max_len // 128))
            self._scratch.append(z(self.lib.onebit_attn_scratch_bytes(ctypes.byref(self._model), S), torch.uint8))
            self._variants["long"] = make_state(short, dict(attn_scratch=self._scratch[-1]), attn_splits=S)
            self.pos.zero_()
            self._warm("long")
        self.pos.zero_()
        self.token.zero_()

    def _launch(self, key, sampled: bool = False):
        """One direct step of variant ``key`` on the current stream."""
        st = ctypes.byref(self._variants[key])
        if sampled:
            _call(self.lib, self.dev, "onebit_decode_step_sampled", ctypes.byref(self._model), st, self._params.data_ptr())
        else:
            _call(self.lib, self.dev, "onebit_decode_step", ctypes.byref(self._model), st)

    def _warm(self, key):
        """The greedy step of variant ``key`` once for real (validates the arguments, sets the kernels' function attributes),
        then its graph."""
        self._launch(key)
        torch.cuda.synchronize(self.dev)
        if self._use_graph:
            self._graphs[(key, False)] = _capture(lambda: self._launch(key))

    def _arm(self, sampling) -> None:
        """Greedy (None) or the given ``SamplingParams`` for the following steps."""
        self._sampled = sampling is not None
        if self._sampled:
            from .sampling import pack
            self._params.copy_(pack([sampling], self.dev))

    @torch.no_grad()
    def prefill(self, input_ids: torch.Tensor) -> torch.Tensor:
        """Run the prompt through the module path into the shared KV cache; returns the fp32 logits
        and arms the engine with the first greedy token."""
        if input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("DecodeEngine is batch 1: input_ids must be [1, S]")
        S = input_ids.shape[1]
        if S + 1 > self.max_len:
            raise ValueError("prompt longer than max_len")
        self.cache.length = 0
        self._sampled = False
        logits = self.model(input_ids.to(self.dev), self.cache)
        self.token.copy_(logits[0, -1].argmax().to(torch.int32).reshape(1))
        self.pos.fill_(S)
        self._prompt_len = S
        self._steps = S
        self.first_token = int(self.token.item())
        return logits

    @torch.no_grad()
    def prime(self, input_ids: torch.Tensor, sampling=None) -> int:
        """The prompt into the KV cache through ``onebit_mixed_step`` (chunks of ``prefill_rows`` tokens, each ONE C call: GEMMs over
        all rows, ragged flash attention with past, lm_head + greedy token on the chunk's last row) and the engine armed with the
        first greedy token, which is returned.  Falls back to ``prefill`` when the native step does not take the model's shape
        (head_dim other than 64 / 128).
        ``sampling`` (``onebit_amd.sampling.SamplingParams``): the first token and every later ``step`` are drawn by the sampler
        (``onebit_mixed_step_sampled``, then the sampled decode graphs); None: greedy."""
        if input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("DecodeEngine is batch 1: input_ids must be [1, S]")
        S = input_ids.shape[1]
        if S < 1 or S + 1 > self.max_len:
            raise ValueError("prompt empty or longer than max_len")
        if self._native_prefill and self._mixed is None:
            try:
                self._mixed = MixedStep(self.model, self.cache.layers, 1, self.max_len, max_rows=min(S, self._prefill_rows))
            except ValueError:
                self._native_prefill = False
        self._arm(sampling)
        if not self._native_prefill:
            logits = self.prefill(input_ids)
            self._arm(sampling)
            if self._sampled:
                from .sampling import sample_logits
                self.token.copy_(sample_logits(logits[0, -1:].half(), self._params, [S]))
                self.first_token = int(self.token.item())
            return self.first_token
        toks = input_ids[0].tolist()
        nxt = None
        for c0 in range(0, S, self._prefill_rows):
            nxt = self._mixed.launch([(0, c0, toks[c0:c0 + self._prefill_rows])], params=self._params if self._sampled else None)
        self.cache.length = S
        self.token.copy_(nxt[:1])
        self.pos.fill_(S)
        self._prompt_len = S
        self._steps = S
        self.first_token = int(self.token.item())
        return self.first_token

    def set_state(self, token: int, pos: int):
        """Arm the engine with ``token`` at cache position ``pos`` (the KV cache must hold ``pos`` tokens)."""
        if not 0 <= int(pos) < self.max_len:
            raise ValueError(f"set_state: position {pos} outside the KV cache [0, {self.max_len})")
        if not 0 <= int(token) < self.cfg.vocab_size:
            raise ValueError(f"set_state: token {token} outside the vocabulary")
        self.token.fill_(int(token))
        self.pos.fill_(int(pos))
        self._steps = int(pos)

    def step(self):
        """Decode one token (asynchronous): consumes the device-side token, appends to the KV cache,
        leaves the next greedy token on the device (sampled, n = position + 1, when ``prime`` armed a ``sampling``).  Raises when the
        KV cache is full: the kernels index the cache, the rope tables and their score buffers by the device-side position."""
        if self._steps >= self.max_len:
            raise RuntimeError(f"DecodeEngine.step: KV cache full ({self.max_len} positions); build the engine with a larger max_len")
        key = step_variant(self._steps, self._long_from, self._short_ok, self._keyblock, self._kb_chunk, self._kb_top)
        g = self._graphs.get((key, self._sampled))
        if g is not None:
            g.replay()
        else:
            self._launch(key, self._sampled)
            if self._sampled and self._use_graph:               # (the greedy graphs were captured at construction)
                self._graphs[(key, True)] = _capture(lambda: self._launch(key, True))
        self._steps += 1

    def logits(self) -> torch.Tensor:
        """fp32 logits of the last step (the reference returns logits.float())."""
        return self.buf["logits"].float()

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, max_new_tokens: int, eos_token_id=None, sampling=None, speculative=None, drafts=None) -> torch.Tensor:
        """Greedy decoding as the reference's ``greedy_search`` (generation/utils.py:2491-2540) for one
        sequence: the prompt followed by up to ``max_new_tokens`` tokens; with ``eos_token_id`` (int or
        list) the output ends with the first EOS token, as the reference's stopping criterion does
        (the steps are enqueued without a host round trip, the cut is made afterwards).  ``sampling``
        (``onebit_amd.sampling.SamplingParams``): sampled decoding instead (token n of the sequence drawn at n, stream
        ``sampling.stream``).  ``speculative`` (``onebit_amd.speculative.SpecConfig``): after the prompt, every pass over the
        weights verifies ``draft_tokens`` prompt-lookup drafts (``SpecStep``) and emits the confirmed ones plus one; the tokens
        are the verify pass's own (argmax, or the sampler's draws), the per-step records ``(n_acc, pos, n_drafted)`` are kept in
        ``self.spec_records``.  ``drafts`` (with ``speculative``): ``drafts(n) -> draft_tokens tokens`` proposed behind a sequence
        of n tokens, in place of the device-side prompt lookup (a caller with a better guess; tests: oracle / adversarial)."""
        S = input_ids.shape[1]
        if S + max_new_tokens > self.max_len:
            raise ValueError(f"generate: prompt {S} + max_new_tokens {max_new_tokens} exceeds the engine's max_len {self.max_len}")
        if speculative is not None:
            return self._generate_speculative(input_ids, max_new_tokens, eos_token_id, sampling, speculative, drafts)
        if drafts is not None:
            raise ValueError("generate: drafts= needs speculative=")
        self.prime(input_ids, sampling=sampling)
        n = max_new_tokens - 1
        for _ in range(max(n, 0)):
            self.step()
        torch.cuda.synchronize(self.dev)
        new: List[int] = [self.first_token] if max_new_tokens > 0 else []
        if n > 0:
            new += self.out_tokens[self._prompt_len:self._prompt_len + n].tolist()
        return self._prompt_and(input_ids, new, eos_token_id)

    def _prompt_and(self, input_ids, new: List[int], eos_token_id) -> torch.Tensor:
        """The prompt followed by the generated tokens up to the first EOS."""
        new = _cut_at_eos(new, eos_token_id)
        return torch.cat([input_ids.to(self.dev), torch.tensor([new], device=self.dev, dtype=input_ids.dtype)], dim=1)

    def _generate_speculative(self, input_ids, max_new_tokens, eos_token_id, sampling, cfg, drafts_fn=None) -> torch.Tensor:
        """``generate`` with speculative steps (``drafts_fn``: ``generate``'s ``drafts``)."""
        S = input_ids.shape[1]
        key = (int(cfg.draft_tokens), int(cfg.ngram_max), int(cfg.ngram_min))
        spec = self._spec_steps.get(key)
        if spec is None:
            chunk = self._kb_chunk if self._keyblock else 64 * max(2, -(-self.max_len // (64 * 64)))
            spec = self._spec_steps[key] = SpecStep(self.model, self.cache.layers, 1, self.max_len, cfg, slot=0, attn_chunk=chunk,
                                                    use_graph=self._use_graph)
        self.prime(input_ids, sampling=sampling)
        self.spec_records = []
        remaining = max_new_tokens - 1
        if remaining > 0:
            spec.arm(sampling)
            spec.seed(input_ids[0].tolist() + [self.first_token], remaining)
            pos = S
            while remaining > 0:
                spec.step(drafts=None if drafts_fn is None else drafts_fn(pos + 1))
                n_acc, pos, n_drafted = spec.read_record()
                self.spec_records.append((n_acc, pos, n_drafted))
                if n_acc < 0:
                    raise RuntimeError("speculative step emitted nothing (KV cache full)")
                remaining -= n_acc + 1
            new = spec.history[S:S + max_new_tokens].tolist()
            self.cache.length = pos
            self.set_state(new[-1], pos)
        else:
            new = [self.first_token] if max_new_tokens > 0 else []
        return self._prompt_and(input_ids, new, eos_token_id)


class BatchedDecodeStep:
    """``onebit_decode_step_batched`` bound to a model and B KV-cache slots: one new token for every
    slot per call (skinny 1-bit GEMMs over the [B, hidden] rows, row-wise glue kernels, attention per
    (head, slot)); the caller owns scheduling, lm_head and sampling.  ``caches[l] = (k, v)`` with k, v
    ``[B, n_kv_heads, max_len, head_dim]`` fp16 on the model's device -- for an fp32 checkpoint build them with
    ``fp16_view(model).new_cache(B, max_len)`` (the model's own ``new_cache`` would be fp32 and is refused)."""

    def __init__(self, model: OneBitLlamaForCausalLM, caches, batch: int, max_len: int, sample: bool = True,
                 keep_logits: bool = False, producer_stats: bool = True, prescaled_rows: bool = True, chains: int = 0,
                 attn_splits: int = 0, attn_chunk: int = 256):
        """``attn_splits`` > 0: attention over key blocks (``onebit_attention_decode_rows``: ``attn_splits`` workgroups of
        ``attn_chunk`` positions per (head, slot)) -- any ``max_len``, and the form to use once contexts pass a few hundred
        positions; ``attn_splits * attn_chunk`` must cover the longest context + 1.  0: one workgroup per (head, slot)."""
        if not 2 <= batch <= 64:
            raise ValueError("batch must be in 2..64")
        self.model, self.cfg, self.dev, self.lib, self._model, self._keep = _bind(model, caches, batch, max_len, "BatchedDecodeStep")
        cfg, dev, self.batch = self.cfg, self.dev, batch
        H, I, D = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
        z = lambda *n: torch.zeros(*n, dtype=torch.float16, device=dev)
        Hq, Hkv = cfg.num_attention_heads * D, cfg.num_key_value_heads * D
        self.tokens = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.pos = torch.full((batch,), -1, dtype=torch.int32, device=dev)
        self.buf = dict(hres0=z(batch, H), hres1=z(batch, H), x=z(batch, H), act=z(batch, I), u_q=z(batch, Hq),
                        u_k=z(batch, Hkv), u_v=z(batch, Hkv), attn_out=z(batch, Hq), u_o=z(batch, H),
                        u_gate=z(batch, I), u_up=z(batch, I), u_down=z(batch, H))
        ptrs, ints = dict(self.buf, tokens=self.tokens, pos=self.pos), dict(batch=batch, chains=int(chains))
        # lm_head + greedy argmax inside the step (the fp16 lm_head streamed once for all rows); needs hidden % 64 == 0
        self.next_tokens = self.logits = None
        if sample and H % 64 == 0:
            self.next_tokens = torch.zeros(batch, dtype=torch.int32, device=dev)
            self._part_val, self._part_idx = _argmax_parts(cfg.vocab_size, dev)
            if keep_logits:
                self.logits = z(batch, cfg.vocab_size)
            ptrs.update(next_tokens=self.next_tokens, logits=self.logits, part_val=self._part_val, part_idx=self._part_idx)
        if attn_splits:
            if attn_chunk < 64 or attn_chunk % 64 or attn_splits < 1:
                raise ValueError("attn_chunk must be a positive multiple of 64, attn_splits >= 1")
            self._q_rows = z(batch, Hq)
            nb = int(self.lib.onebit_attention_decode_scratch_bytes(batch, cfg.num_attention_heads, int(attn_splits)))
            self._attn_scratch = torch.zeros(max(nb, 16), dtype=torch.uint8, device=dev)
            ptrs.update(q_rows=self._q_rows, attn_scratch=self._attn_scratch)
            ints.update(attn_splits=int(attn_splits), attn_chunk=int(attn_chunk))
        # room for the consumers' pre-scaled rows fp16(x * input_factor): the projections then take the LDS-DMA skinny GEMM
        if prescaled_rows:
            self._x_scaled = ptrs["x_scaled"] = z(3, batch, H)
        # scratch for the q|k|v LayerNorm partials (published by the GEMM, combined by the attention workgroups)
        if producer_stats:
            nst = int(self.lib.onebit_batch_stats_floats(ctypes.byref(self._model), batch))
            self._qkv_stats = ptrs["qkv_stats"] = torch.zeros(max(nst, 1), dtype=torch.float32, device=dev)
        self._state = make_state(_BatchState, ptrs, **ints)
        self._state_s = None            # the sampled form's copy of the state (with logits), made on first use

    def _sampled_state(self):
        if self._state_s is None:
            if self.next_tokens is None:
                raise ValueError("BatchedDecodeStep: the sampled step needs sample=True")
            if self.logits is None:
                self.logits = torch.zeros(self.batch, self.cfg.vocab_size, dtype=torch.float16, device=self.dev)
            self._state_s = make_state(self._state, dict(logits=self.logits))
        return self._state_s

    def launch(self, params: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Enqueue one step on the current stream; returns the final-norm output x [B, hidden]
        (a view of a persistent buffer).  With ``sample`` the greedy next token of every slot is in
        ``self.next_tokens`` (int32 [B]) afterwards, computed by the same call.  ``params``: device rows of
        onebit_sample_params_t (``sampling.pack``, uint8 [B, 32]) -- the tokens are drawn by the sampler instead
        (``onebit_decode_step_batched_sampled``, n = pos[b] + 1; needs ``sample``).  The sampled form writes the logits to
        ``self.logits``, allocated on its first use without ``keep_logits`` (the greedy form keeps its own state)."""
        if params is None:
            _call(self.lib, self.dev, "onebit_decode_step_batched", ctypes.byref(self._model), ctypes.byref(self._state))
        else:
            _check_params(params, self.batch, self.dev)
            _call(self.lib, self.dev, "onebit_decode_step_batched_sampled", ctypes.byref(self._model), ctypes.byref(self._sampled_state()),
                  params.data_ptr())
        return self.buf["x"]


class MixedStep:
    """``onebit_mixed_step`` bound to a model and its KV-cache slots: ONE scheduler step of continuous batching (BASELINE config 5)
    on native kernels -- the token rows of all scheduled items concatenated, every 1-bit projection one GEMM over all rows, fused
    row glue, ragged attention (prompt chunks: causal flash attention with past; single-token rows: split-KV decode attention),
    lm_head + greedy token on the last row of every item.  ``caches[l] = (k, v)``, ``[n_slots, n_kv_heads, max_len, head_dim]``
    fp16.  The reference has no counterpart for the batching; per row the arithmetic is modeling_bitllama.py:869-918, 487-585."""

    def __init__(self, model: OneBitLlamaForCausalLM, caches, n_slots: int, max_len: int, max_rows: int = 4096,
                 attn_chunk: int = 256, keep_logits: bool = False):
        self.model, self.cfg, self.dev, self.lib, self._model, self._keep = _bind(model, caches, n_slots, max_len, "MixedStep")
        cfg = self.cfg
        if cfg.head_dim not in (64, 128) or cfg.hidden_size % 64 != 0 or cfg.num_attention_heads * cfg.head_dim != cfg.hidden_size:
            raise ValueError("MixedStep: head_dim must be 64 or 128 and hidden a multiple of 64")
        self.n_slots, self.max_len, self.attn_chunk = int(n_slots), int(max_len), int(attn_chunk)
        if -(-self.max_len // self.attn_chunk) > 64:
            raise ValueError("MixedStep: attn_chunk too small for max_len (at most 64 splits)")
        self._part_val, self._part_idx = _argmax_parts(cfg.vocab_size, self.dev)
        self.keep_logits = keep_logits
        self.logits = None
        self._rows = 0
        self._ensure(int(max_rows))
        self.launches = 0

    def _ensure(self, rows: int):
        """Room for a step of ``rows`` token rows (staging rows, workspace); grows geometrically, never shrinks."""
        if rows <= self._rows:
            return
        rows = max(rows, 2 * self._rows, 64)
        dev, ns = self.dev, self.n_slots
        nb = int(self.lib.onebit_mixed_workspace_bytes(ctypes.byref(self._model), rows, ns, self.attn_chunk))
        self._ws = None                                           # (free the old block first)
        self._ws, self._ws_off = _aligned_ws(nb, dev)
        # one pinned staging row [tokens | row_slot | row_pos | out_rows] and ONE asynchronous copy per step; two of them in turn,
        # each guarded by an event, so that a caller who enqueues steps without synchronising never rewrites a row in flight
        self._h_stage = [torch.zeros(4 * rows + ns, dtype=torch.int32).pin_memory() for _ in range(2)]
        self._h_np = [h.numpy() for h in self._h_stage]
        self._h_ev = [None, None]
        self._d_stage = [torch.zeros(4 * rows + ns, dtype=torch.int32, device=dev) for _ in range(2)]
        self.next_tokens = torch.zeros(rows + ns, dtype=torch.int32, device=dev)
        self._rows = rows
        self._ensure_logits(ns)

    def _ensure_logits(self, n: int, need: bool = False):
        if (self.keep_logits or need or self.logits is not None) and (self.logits is None or self.logits.shape[0] < n):
            self.logits = None
            self.logits = torch.zeros(max(n, self.n_slots), self.cfg.vocab_size, dtype=torch.float16, device=self.dev)

    @torch.no_grad()
    def launch(self, items, params: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Enqueue one step on the current stream.  ``items``: ``(slot, start, tokens)`` per scheduled request (distinct slots):
        ``tokens`` enter the request's cache slot at positions ``start ...``.  Returns the device tensor of greedy next tokens,
        one per item in the order given (the token after the item's LAST row: for a prompt chunk that is not the prompt's last one
        the caller ignores it).  An item may carry a fourth element ``k`` (default 1): lm_head runs on its last ``k`` rows (the
        evaluation caller scores a request's continuation rows) and the item contributes ``k`` consecutive entries to the returned
        tokens and to ``logits``.  Asynchronous: synchronise before reading.
        ``params``: device rows of onebit_sample_params_t (``sampling.pack``, uint8 [n_out, 32], in the order of the returned
        tokens): the tokens are drawn by the sampler (``onebit_mixed_step_sampled``, n = the row's position + 1; needs
        logits: they go to ``self.logits``, allocated on first use)."""
        n_items = len(items)
        if n_items == 0 or n_items > self.n_slots:
            raise ValueError(f"MixedStep.launch: {n_items} items for {self.n_slots} slots")
        T = sum(len(it[2]) for it in items)
        self._ensure(T)
        R, ns, V = self._rows, self.n_slots, self.cfg.vocab_size
        sb = self.launches & 1
        if self._h_ev[sb] is not None:
            self._h_ev[sb].synchronize()
        st = self._h_np[sb]
        tok, rs, rp, outr = st[:R], st[R:2 * R], st[2 * R:3 * R], st[3 * R:]
        order = sorted(range(n_items), key=lambda i: len(items[i][2]) != 1)          # single-token rows first (stable)
        outs = [int(it[3]) if len(it) > 3 else 1 for it in items]
        out0 = [0] * n_items
        for i in range(1, n_items):
            out0[i] = out0[i - 1] + outs[i - 1]
        n_out = out0[-1] + outs[-1]
        self._ensure_logits(n_out, need=params is not None)
        segs, row, n_dec, dec_ctx, seen = [], 0, 0, 0, set()
        for i in order:
            slot, start, toks = items[i][:3]
            n = len(toks)
            if not 1 <= outs[i] <= n:
                raise ValueError(f"MixedStep.launch: item {i} asks for {outs[i]} output rows of {n}")
            if n < 1 or not 0 <= slot < ns or start < 0 or start + n > self.max_len or slot in seen:
                raise ValueError(f"MixedStep.launch: item {i} (slot {slot}, start {start}, {n} tokens) outside the cache or a repeated slot")
            if min(toks) < 0 or max(toks) >= V:
                raise ValueError(f"MixedStep.launch: item {i} has a token outside the vocabulary")
            seen.add(slot)
            tok[row:row + n] = toks
            rs[row:row + n] = slot
            rp[row:row + n] = range(start, start + n)
            if n == 1:
                n_dec += 1
                dec_ctx = max(dec_ctx, start + 1)
            else:
                segs.append((row, n, slot, start))
            outr[out0[i]:out0[i] + outs[i]] = range(row + n - outs[i], row + n)
            row += n
        d = self._d_stage[sb]
        d.copy_(self._h_stage[sb], non_blocking=True)                                # stream-ordered before the kernels
        self._h_ev[sb] = torch.cuda.Event()
        self._h_ev[sb].record(torch.cuda.current_stream(self.dev))
        seg_arr = (_Seg * max(len(segs), 1))(*[_Seg(*g) for g in segs])
        base = d.data_ptr()
        state = make_state(
            _MixedState, dict(next_tokens=self.next_tokens, part_val=self._part_val, part_idx=self._part_idx,
                              logits=self.logits if self.keep_logits or params is not None else None),
            n_rows=T, n_dec=n_dec, n_seg=len(segs), n_out=n_out, n_slots=ns, attn_chunk=self.attn_chunk, dec_ctx=dec_ctx,
            tokens=base, row_slot=base + 4 * R, row_pos=base + 8 * R, out_rows=base + 12 * R, segs=seg_arr,
            workspace=self._ws.data_ptr() + self._ws_off, workspace_bytes=self._ws.numel() - self._ws_off)
        if params is None:
            _call(self.lib, self.dev, "onebit_mixed_step", ctypes.byref(self._model), ctypes.byref(state))
        else:
            _check_params(params, n_out, self.dev)
            _call(self.lib, self.dev, "onebit_mixed_step_sampled", ctypes.byref(self._model), ctypes.byref(state), params.data_ptr())
        self.launches += 1
        return self.next_tokens[:n_out]


class SpecStep:
    """``onebit_spec_step`` bound to a model and ONE slot of its KV caches: a speculative decode step -- the sequence's last token
    and ``k`` draft tokens as k + 1 rows through the mixed step's layer body, multi-query key-block attention
    (``onebit_attention_decode_rows_mq``), lm_head + argmax (or the sampler) on every row, then the commit kernel: accept the
    confirmed drafts, append the emitted tokens to ``history``, draft the next step by prompt lookup (``speculative.propose`` /
    ``accept`` state the contract).  Everything a step reads is on the device; one HIP graph per (split count, greedy | sampled)
    is captured on its second use.  The host reads the 12-byte commit record once per step (``read_record``) to pick the next
    step's split count and to stop."""

    def __init__(self, model: OneBitLlamaForCausalLM, caches, n_slots: int, max_len: int, cfg, slot: int = 0,
                 attn_chunk: int = 128, keep_logits: bool = False, use_graph: bool = True):
        self.model, self.cfg, self.dev, self.lib, self._model, self._keep = _bind(model, caches, n_slots, max_len, "SpecStep")
        mc = self.cfg
        if mc.head_dim not in (64, 128) or mc.hidden_size % 64 != 0 or mc.num_attention_heads * mc.head_dim != mc.hidden_size:
            raise ValueError("SpecStep: head_dim must be 64 or 128 and hidden a multiple of 64")
        if max_len > 15360:
            raise ValueError("SpecStep: max_len above 15360 (the commit kernel searches the token history in LDS)")
        if attn_chunk < 64 or attn_chunk % 64 or -(-max_len // attn_chunk) > 64:
            raise ValueError("SpecStep: attn_chunk must be a multiple of 64 with at most 64 splits over max_len")
        if not 0 <= slot < n_slots:
            raise ValueError("SpecStep: slot outside the caches")
        self.k, self.ngram_max, self.ngram_min = int(cfg.draft_tokens), int(cfg.ngram_max), int(cfg.ngram_min)
        self.n_slots, self.max_len, self.slot, self.attn_chunk = int(n_slots), int(max_len), int(slot), int(attn_chunk)
        dev, k = self.dev, self.k
        # one int32 block: tokens[16] | row_slot[16] | row_pos[16] | drafts[16] | chosen[16] | pos, remaining, -, - | record[4]
        self._ints = torch.zeros(88, dtype=torch.int32, device=dev)
        self._ints[16:32] = self.slot
        self._h_ints = torch.zeros(88, dtype=torch.int32).pin_memory()
        self._h_drafts = torch.zeros(16, dtype=torch.int32).pin_memory()
        self.tokens, self.row_pos, self.drafts = self._ints[0:k + 1], self._ints[32:33 + k], self._ints[48:48 + k]
        self.chosen, self.pos, self.remaining, self._rec_dev = self._ints[64:65 + k], self._ints[80:81], self._ints[81:82], self._ints[84:87]
        self.history = torch.zeros(self.max_len, dtype=torch.int32, device=dev)
        self._rec_host = torch.zeros(3, dtype=torch.int32).pin_memory()
        self._part_val, self._part_idx = _argmax_parts(mc.vocab_size, dev)
        self.keep_logits = bool(keep_logits)
        self.logits = torch.zeros(k + 1, mc.vocab_size, dtype=torch.float16, device=dev)
        nb = int(self.lib.onebit_spec_workspace_bytes(ctypes.byref(self._model), k, self.attn_chunk))
        if nb == 0:
            raise ValueError("SpecStep: onebit_spec_workspace_bytes refused the model")
        self._ws, self._ws_off = _aligned_ws(nb, dev)
        self._params = torch.zeros(k + 1, 32, dtype=torch.uint8, device=dev)
        self._sampled = False
        self._use_graph = bool(use_graph)
        self._states, self._graphs, self._seen = {}, {}, set()
        self._host_pos = 0
        self.read_back = True           # probes: False leaves the record on the device (no copy, the caller must not read it)
        self.steps = 0

    def _state(self, ns: int, sampled: bool) -> _SpecState:
        st = self._states.get((ns, sampled))
        if st is None:
            base = self._ints.data_ptr()        # (byte offsets into the int32 block laid out in __init__)
            st = self._states[(ns, sampled)] = make_state(
                _SpecState, dict(history=self.history, logits=self.logits if sampled or self.keep_logits else None,
                                 part_val=self._part_val, part_idx=self._part_idx),
                k=self.k, n_slots=self.n_slots, attn_chunk=self.attn_chunk, attn_splits=ns, ngram_max=self.ngram_max, ngram_min=self.ngram_min,
                tokens=base, row_slot=base + 4 * 16, row_pos=base + 4 * 32, drafts=base + 4 * 48, chosen=base + 4 * 64,
                pos=base + 4 * 80, remaining=base + 4 * 81, record=base + 4 * 84,
                workspace=self._ws.data_ptr() + self._ws_off, workspace_bytes=self._ws.numel() - self._ws_off)
        return st

    def splits(self, ctx: int) -> int:
        """Power-of-two split count whose splits * attn_chunk positions cover ``ctx`` keys (at most 64)."""
        ns = 1
        while ns * self.attn_chunk < ctx and ns < 64:
            ns *= 2
        return ns

    def arm(self, sampling) -> None:
        """Greedy (None) or the given ``SamplingParams`` for the following steps (every row draws with the request's row)."""
        self._sampled = sampling is not None
        if self._sampled:
            from .sampling import pack
            self._params.copy_(pack([sampling] * (self.k + 1), self.dev))

    def seed(self, history, remaining: int, drafts=None) -> None:
        """The sequence so far (its KV cache holds all but the last token; the last token is the next step's first row) and the
        number of tokens still to emit.  The first step's drafts: ``speculative.propose`` on the host, or ``drafts``."""
        from .speculative import propose
        n = len(history)
        if not 1 <= n <= self.max_len:
            raise ValueError("SpecStep.seed: history empty or longer than max_len")
        if min(history) < 0 or max(history) >= self.cfg.vocab_size:
            raise ValueError("SpecStep.seed: token outside the vocabulary")
        k, P = self.k, n - 1
        d = list(drafts) if drafts is not None else propose(history, k, self.ngram_max, self.ngram_min)[0]
        if len(d) != k:
            raise ValueError(f"SpecStep.seed: {len(d)} drafts for k = {k}")
        torch.cuda.current_stream(self.dev).synchronize()          # (the pinned staging block may still be in flight)
        h = self._h_ints.numpy()
        h[:] = 0
        h[0], h[1:k + 1] = history[-1], d
        h[16:32] = self.slot
        h[32:33 + k] = range(P, P + k + 1)
        h[48:48 + k] = d
        h[80], h[81] = P, int(remaining)
        self._ints.copy_(self._h_ints, non_blocking=True)
        self.history[:n].copy_(torch.tensor(list(history), dtype=torch.int32), non_blocking=False)
        self._host_pos = P

    def set_drafts(self, drafts) -> None:
        """Replace the next step's drafts (teacher forcing, oracle / adversarial drafts)."""
        d = [int(t) for t in drafts]
        if len(d) != self.k or min(d) < 0 or max(d) >= self.cfg.vocab_size:
            raise ValueError(f"SpecStep: need {self.k} draft tokens inside the vocabulary")
        torch.cuda.current_stream(self.dev).synchronize()          # (the pinned staging row may still be in flight)
        self._h_drafts.numpy()[:self.k] = d
        self._ints[1:self.k + 1].copy_(self._h_drafts[:self.k], non_blocking=True)
        self._ints[48:48 + self.k].copy_(self._h_drafts[:self.k], non_blocking=True)

    def _launch(self, st, sampled: bool):
        if sampled:
            _call(self.lib, self.dev, "onebit_spec_step_sampled", ctypes.byref(self._model), ctypes.byref(st), self._params.data_ptr())
        else:
            _call(self.lib, self.dev, "onebit_spec_step", ctypes.byref(self._model), ctypes.byref(st))
        if self.read_back:
            self._rec_host.copy_(self._rec_dev, non_blocking=True)

    def step(self, drafts=None, ns: Optional[int] = None) -> None:
        """Enqueue one speculative step (asynchronous).  ``ns``: attention splits (default: what covers the host-known position
        + k + 1 keys).  ``drafts``: override the device-side drafts of this step."""
        if drafts is not None:
            self.set_drafts(drafts)
        if ns is None:
            ns = self.splits(self._host_pos + self.k + 1)
        key = (ns, self._sampled, self.read_back)
        g = self._graphs.get(key)
        if g is not None:
            g.replay()
        else:
            st = self._state(ns, self._sampled)
            self._launch(st, self._sampled)                        # this step; its graph is captured for the next ones
            if self._use_graph and key in self._seen:
                self._graphs[key] = _capture(lambda: self._launch(st, self._sampled))
            self._seen.add(key)
        self.steps += 1

    def read_record(self):
        """Wait for the enqueued steps and return the last one's commit record ``(n_acc, pos, n_drafted)``: the step emitted
        ``n_acc + 1`` tokens (-1: nothing -- no budget or the cache is full), ``pos`` is the position of the sequence's last token."""
        torch.cuda.current_stream(self.dev).synchronize()
        r = self._rec_host.numpy()
        self._host_pos = int(r[1])
        return int(r[0]), int(r[1]), int(r[2])
