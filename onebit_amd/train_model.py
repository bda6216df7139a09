"""Train-mode OneBit LLaMA on MI355X: the student that ``KDLoss`` is computed on and that ``python -m onebit_amd.svid`` builds
start checkpoints for.

``OneBitLlamaForCausalLMTrain`` restates the reference's ``BitLlamaForCausalLM`` (``modeling_bitllama.py:1338-``) ->
``LlamaModel`` (``:1040-1187``) -> ``LlamaDecoderLayer`` (``:781-853``) -> ``LlamaAttention`` (``:274-429``) / ``LlamaMLP``
(``:184-221``) with the reference's module names, so the state-dict keys are ``BitLlamaForCausalLM``'s: a start checkpoint from
``svid.build_start_state_dict`` loads with ``strict=True`` and ``checkpoint.convert_train_state_dict(model.state_dict())`` loads
into the packed ``OneBitLlamaForCausalLM``.

What runs where: the seven projections of a layer are ``train.BitLinear`` (HIP forward and ``SignSTE`` backward); the attention
is ``flash_attention_train`` -- hand-written HIP kernels behind ``onebit_attention_train_forward`` / ``_backward``
(``csrc/ob_flash_train.h``): flash style in BOTH directions, nothing of size ``S^2`` is formed or saved, no atomics, so the
gradients are bit-reproducible.  RMSNorm, RoPE, SwiGLU, the residual adds, ``embed_tokens``, ``lm_head`` and the cross-entropy
are torch ops under autograd in the reference's op order; fusing them is a later change.  As in the reference, ``embed_tokens``
(``:1053``), ``lm_head`` (``:1346``) and the RMSNorm weights (``:73``) are frozen; the 1-bit projections are what trains.

``attention="hip"`` (default) needs float16 on the GPU.  ``attention="eager"`` is the reference's op order (``:389-406``:
scores / sqrt(D) + mask, softmax in fp32, probabilities cast back) written in torch for float32 and float16: the route of
float32 models and, with ``BitLinear``'s float32 kernels, the parity route.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn
from torch.autograd.function import once_differentiable
from torch.utils.checkpoint import checkpoint as _checkpoint

from . import _lib
from .bitnet import _require_gpu, _stream_ptr
from .llama import LlamaRMSNorm, OneBitLlamaConfig, _rotate_half, rope_tables
from .train import BitLinear

__all__ = ["flash_attention_train", "eager_attention_train", "LlamaMLP", "LlamaAttention", "LlamaDecoderLayer", "LlamaModel",
           "OneBitLlamaForCausalLMTrain"]


class _FlashAttnTrainFn(torch.autograd.Function):
    """Saves q, k, v, o (fp16) and lse (fp32 [B, H, S]); nothing of size S^2."""

    @staticmethod
    def forward(ctx, q, k, v):
        B, S, H, D = q.shape
        Hkv = k.shape[2]
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        o = torch.empty_like(q)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
        with torch.cuda.device(q.device):
            rc = _lib.load().onebit_attention_train_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
                                                            B, S, H, Hkv, D, _stream_ptr(q.device))
        _lib.check(rc, "onebit_attention_train_forward")
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.mark_non_differentiable(lse)
        return o, lse

    @staticmethod
    @once_differentiable               # the gradients come out of a C-ABI call: no graph behind them, no double backward
    def backward(ctx, d_o, _d_lse):
        q, k, v, o, lse = ctx.saved_tensors
        B, S, H, D = q.shape
        Hkv = k.shape[2]
        d_o = d_o.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        lib = _lib.load()
        nws = lib.onebit_attention_train_workspace_bytes(B, S, H, Hkv, D)
        ws = torch.empty(nws, dtype=torch.uint8, device=q.device)
        with torch.cuda.device(q.device):
            rc = lib.onebit_attention_train_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), d_o.data_ptr(),
                                                     dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), nws, B, S, H, Hkv, D,
                                                     _stream_ptr(q.device))
        _lib.check(rc, "onebit_attention_train_backward")
        return dq, dk, dv


def _check_qkv(q, k, v, what):
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[1] != k.shape[1] or q.shape[3] != k.shape[3]:
        raise ValueError(f"{what}: expected q [B, S, H, D] and k, v [B, S, Hkv, D], got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    if k.shape[2] == 0 or q.shape[2] % k.shape[2]:
        raise ValueError(f"{what}: {q.shape[2]} query heads are not a multiple of {k.shape[2]} kv heads")


def flash_attention_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, return_lse: bool = False):
    """Causal self-attention ``softmax(q k^T / sqrt(D) + causal mask) v`` of token-major ``q [B, S, H, D]`` and ``k, v [B, S, Hkv, D]``
    (float16, GPU, D 64 or 128, Hkv dividing H) -> ``[B, S, H, D]``, differentiable w.r.t. all three.  ``return_lse``: also the
    fp32 log-sum-exp ``[B, H, S]`` (not differentiable)."""
    for t in (q, k, v):
        _require_gpu(t, "flash_attention_train")
    _check_qkv(q, k, v, "flash_attention_train")
    if not (q.dtype == k.dtype == v.dtype == torch.float16):
        raise RuntimeError("flash_attention_train: float16 only (attention='eager' is the route for float32)")
    o, lse = _FlashAttnTrainFn.apply(q, k, v)
    return (o, lse) if return_lse else o


def eager_attention_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """The same function in the reference's op order (``modeling_bitllama.py:386-414``) on torch ops, same layout in and out:
    scores / sqrt(D) + the additive causal mask in the tensor dtype, softmax in fp32, probabilities cast back, times v."""
    _check_qkv(q, k, v, "eager_attention_train")
    B, S, H, D = q.shape
    rep = H // k.shape[2]
    qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    if rep != 1:
        kt, vt = kt.repeat_interleave(rep, dim=1), vt.repeat_interleave(rep, dim=1)
    w = torch.matmul(qt, kt.transpose(2, 3)) / math.sqrt(D)
    mask = torch.triu(torch.full((S, S), torch.finfo(w.dtype).min, device=w.device, dtype=w.dtype), diagonal=1)
    w = w + mask[None, None]
    w = nn.functional.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
    return torch.matmul(w, vt).transpose(1, 2).contiguous()


class LlamaMLP(nn.Module):
    """modeling_bitllama.py:184-221."""

    def __init__(self, config: OneBitLlamaConfig, dtype=None):
        super().__init__()
        self.gate_proj = BitLinear(config.hidden_size, config.intermediate_size, bias=False, dtype=dtype)
        self.up_proj = BitLinear(config.hidden_size, config.intermediate_size, bias=False, dtype=dtype)
        self.down_proj = BitLinear(config.intermediate_size, config.hidden_size, bias=False, dtype=dtype)

    def forward(self, x):
        return self.down_proj(nn.functional.silu(self.gate_proj(x)) * self.up_proj(x))


class LlamaAttention(nn.Module):
    """modeling_bitllama.py:274-429 without a cache.  q, k, v stay in the projections' token-major layout [B, S, heads, D]."""

    def __init__(self, config: OneBitLlamaConfig, dtype=None, attention: str = "hip"):
        super().__init__()
        H, Hkv, D = config.num_attention_heads, config.num_key_value_heads, config.head_dim
        self.num_heads, self.num_key_value_heads, self.head_dim, self.hidden_size = H, Hkv, D, config.hidden_size
        self.q_proj = BitLinear(self.hidden_size, H * D, bias=config.attention_bias, dtype=dtype)
        self.k_proj = BitLinear(self.hidden_size, Hkv * D, bias=config.attention_bias, dtype=dtype)
        self.v_proj = BitLinear(self.hidden_size, Hkv * D, bias=config.attention_bias, dtype=dtype)
        self.o_proj = BitLinear(H * D, self.hidden_size, bias=config.attention_bias, dtype=dtype)
        self.attn_impl = attention

    def forward(self, hidden_states, cos, sin):
        B, S, _ = hidden_states.shape
        H, Hkv, D = self.num_heads, self.num_key_value_heads, self.head_dim
        q = self.q_proj(hidden_states).view(B, S, H, D)
        k = self.k_proj(hidden_states).view(B, S, Hkv, D)
        v = self.v_proj(hidden_states).view(B, S, Hkv, D)
        c, s = cos[:S][None, :, None, :], sin[:S][None, :, None, :]
        q = (q * c) + (_rotate_half(q) * s)                  # apply_rotary_pos_emb, :175-181
        k = (k * c) + (_rotate_half(k) * s)
        if self.attn_impl == "hip":
            if q.dtype != torch.float16:
                raise RuntimeError("attention='hip' is float16 only; build the model with attention='eager' for float32")
            o = flash_attention_train(q, k, v)
        else:
            o = eager_attention_train(q, k, v)
        return self.o_proj(o.reshape(B, S, H * D))


class LlamaDecoderLayer(nn.Module):
    """modeling_bitllama.py:781-853."""

    def __init__(self, config: OneBitLlamaConfig, dtype=None, attention: str = "hip"):
        super().__init__()
        self.self_attn = LlamaAttention(config, dtype, attention)
        self.mlp = LlamaMLP(config, dtype)
        self.input_layernorm = LlamaRMSNorm(config.hidden_size, eps=config.rms_norm_eps, dtype=dtype)
        self.post_attention_layernorm = LlamaRMSNorm(config.hidden_size, eps=config.rms_norm_eps, dtype=dtype)

    def forward(self, h, cos, sin):
        h = h + self.self_attn(self.input_layernorm(h), cos, sin)
        h = h + self.mlp(self.post_attention_layernorm(h))
        return h


class LlamaModel(nn.Module):
    """modeling_bitllama.py:1040-1187: frozen embedding (:1053), the layers, the final norm."""

    def __init__(self, config: OneBitLlamaConfig, dtype=None, attention: str = "hip"):
        super().__init__()
        self.embed_tokens = nn.Embedding(config.vocab_size, config.hidden_size, dtype=dtype)
        self.embed_tokens.weight.requires_grad_(False)
        self.layers = nn.ModuleList([LlamaDecoderLayer(config, dtype, attention) for _ in range(config.num_hidden_layers)])
        self.norm = LlamaRMSNorm(config.hidden_size, eps=config.rms_norm_eps, dtype=dtype)
        self.gradient_checkpointing = False

    def forward(self, input_ids, cos, sin, output_hidden_states: bool = False):
        h = self.embed_tokens(input_ids)
        states = []
        for layer in self.layers:
            if output_hidden_states:
                states.append(h)
            if self.gradient_checkpointing and torch.is_grad_enabled():
                # the layer runs again in backward; its kernels are deterministic, so the gradients are bit-identical
                h = _checkpoint(layer, h, cos, sin, use_reentrant=False)
            else:
                h = layer(h, cos, sin)
        h = self.norm(h)
        if output_hidden_states:
            states.append(h)
        return h, (tuple(states) if output_hidden_states else None)


class OneBitLlamaForCausalLMTrain(nn.Module):
    """``BitLlamaForCausalLM`` (modeling_bitllama.py:1338-): see the module docstring.

    ``forward(input_ids, labels=None, output_hidden_states=False)`` returns ``(logits, hidden_states, loss)``: float32 logits
    ``[B, S, vocab]`` (``.float()`` of the lm_head output, :1437); the ``L + 1`` hidden states in the reference's order -- the
    embedding output first, each layer's input after it, the final norm's output last (:1131-1165) -- or ``None``; the shifted
    cross-entropy (:1441-1450) or ``None`` without ``labels``."""

    def __init__(self, config: OneBitLlamaConfig, dtype=torch.float16, attention: Optional[str] = None,
                 gradient_checkpointing: bool = False):
        super().__init__()
        if attention is None:
            attention = "hip" if dtype == torch.float16 else "eager"
        if attention not in ("hip", "eager"):
            raise ValueError("attention must be 'hip' or 'eager'")
        if attention == "hip" and dtype != torch.float16:
            raise RuntimeError("attention='hip' is float16 only; use attention='eager' for float32")
        if attention == "hip" and config.head_dim not in (64, 128):
            raise ValueError(f"attention='hip' supports head_dim 64 and 128, got {config.head_dim}")
        self.config, self.attention = config, attention
        self.model = LlamaModel(config, dtype, attention)
        self.model.gradient_checkpointing = bool(gradient_checkpointing)
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False, dtype=dtype)
        self.lm_head.weight.requires_grad_(False)            # :1346
        self._rope = None

    @property
    def gradient_checkpointing(self) -> bool:
        return self.model.gradient_checkpointing

    @gradient_checkpointing.setter
    def gradient_checkpointing(self, on: bool):
        self.model.gradient_checkpointing = bool(on)

    def _rope_tables(self, device, dtype, seq_len: int):
        """grown on demand as ``OneBitLlamaForCausalLM._rope_tables`` does, ``rope_scaling`` included"""
        cfg = self.config
        have = 0 if self._rope is None else self._rope[0].shape[0]
        need = max(cfg.max_position_embeddings, seq_len, have)
        if self._rope is None or self._rope[0].device != device or self._rope[0].dtype != dtype or need > have:
            self._rope = rope_tables(cfg.head_dim, cfg.max_position_embeddings, cfg.rope_theta, device, dtype, seq_len=need,
                                     scaling=cfg.rope_scaling)
        return self._rope

    def forward(self, input_ids: torch.Tensor, labels: Optional[torch.Tensor] = None, output_hidden_states: bool = False,
                output_attentions: bool = False):
        if output_attentions:
            raise NotImplementedError(
                "kd_gamma > 0 (the attention-weight term) needs materialised [B, H, S, S] attention weights; "
                "this project's attention kernels never form them")
        _require_gpu(input_ids, "OneBitLlamaForCausalLMTrain.forward")
        _require_gpu(self.lm_head.weight, "OneBitLlamaForCausalLMTrain.forward (parameters)")
        if input_ids.dim() != 2:
            raise ValueError("input_ids must be [B, S]")
        w = self.lm_head.weight
        cos, sin = self._rope_tables(w.device, w.dtype, input_ids.shape[1])
        h, states = self.model(input_ids, cos, sin, output_hidden_states)
        logits = self.lm_head(h).float()
        loss = None
        if labels is not None:
            V = logits.shape[-1]
            loss = nn.functional.cross_entropy(logits[..., :-1, :].contiguous().view(-1, V), labels[..., 1:].contiguous().view(-1).to(logits.device))
        return logits, states, loss

    @classmethod
    def from_teacher_state_dict(cls, config: OneBitLlamaConfig, teacher_sd, dtype=torch.float16, device="cuda", progress=None,
                                **kwargs) -> "OneBitLlamaForCausalLMTrain":
        """A dense LLaMA teacher's state dict -> a student at its SVID start point: ``svid.build_start_state_dict`` on ``device``
        (latent ``sign * 0.01`` weights, ``weight_scale``, ``input_factor``), the teacher's own embedding, norm and lm_head
        tensors, loaded with ``strict=True``."""
        from .svid import build_start_state_dict
        sd = build_start_state_dict(teacher_sd, device=device, progress=progress)
        sd = {k: v.to(dtype) for k, v in sd.items() if "rotary_emb.inv_freq" not in k}
        model = cls(config, dtype=dtype, **kwargs)
        model.load_state_dict(sd, strict=True)
        return model.to(device)
