"""ctypes mirrors of the structs of include/onebit.h, and the one way they are filled.

Every mirror's field list is compared with the header by tests/test_abi_cpu.py (the library's ``struct_size`` check sees the
total size only).  The functions themselves are typed in ``_lib.SYMBOLS`` and nowhere else: struct pointers go in as
``ctypes.byref(x)``, struct arrays as ``ctypes.cast(arr, c_void_p)``.
"""
from __future__ import annotations

import ctypes
import functools

import torch

_vp, _i64, _i32, _f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float


class _Proj(ctypes.Structure):
    _fields_ = [("weight", _vp), ("input_factor", _vp), ("weight_scale", _vp),
                ("N", _i64), ("K", _i64), ("ldw_bytes", _i64)]


class _Layer(ctypes.Structure):
    _fields_ = [("q", _Proj), ("k", _Proj), ("v", _Proj), ("o", _Proj), ("gate", _Proj), ("up", _Proj),
                ("down", _Proj), ("input_layernorm_w", _vp), ("post_attention_layernorm_w", _vp),
                ("k_cache", _vp), ("v_cache", _vp),
                ("q_bias", _vp), ("k_bias", _vp), ("v_bias", _vp), ("o_bias", _vp)]          # ABI 8: config.attention_bias


class _Model(ctypes.Structure):
    _fields_ = [("n_layers", _i32), ("hidden", _i32), ("intermediate", _i32), ("n_heads", _i32),
                ("n_kv_heads", _i32), ("head_dim", _i32), ("vocab", _i32), ("max_len", _i32),
                ("rms_eps", _f), ("ln_eps", _f), ("layers", ctypes.POINTER(_Layer)),
                ("embed", _vp), ("final_norm_w", _vp), ("lm_head", _vp), ("rope_cos", _vp), ("rope_sin", _vp)]


class _State(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint64),      # ABI 8: checked by the library (a state of another ABI is refused, not misread)
                ("token", _vp), ("pos", _vp), ("out_tokens", _vp), ("max_out", _i32),
                ("hres0", _vp), ("hres1", _vp), ("u_q", _vp), ("u_k", _vp), ("u_v", _vp),
                ("attn_out", _vp), ("u_o", _vp), ("u_gate", _vp), ("u_up", _vp), ("u_down", _vp),
                ("logits", _vp), ("part_val", _vp), ("part_idx", _vp), ("attn_splits", _i32), ("attn_scratch", _vp),
                ("tile_stats", _vp), ("rope_cur", _vp), ("attn_blind", _i32),
                ("attn_chunk", _i32), ("q_rows", _vp)]                                   # ABI 9: key-block long-context attention


class _BatchState(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint64), ("batch", _i32), ("tokens", _vp), ("pos", _vp), ("hres0", _vp), ("hres1", _vp), ("x", _vp),
                ("act", _vp), ("u_q", _vp), ("u_k", _vp), ("u_v", _vp), ("attn_out", _vp), ("u_o", _vp),
                ("u_gate", _vp), ("u_up", _vp), ("u_down", _vp),
                ("next_tokens", _vp), ("logits", _vp), ("part_val", _vp), ("part_idx", _vp), ("qkv_stats", _vp),
                ("x_scaled", _vp), ("chains", _i32),
                ("attn_splits", _i32), ("attn_chunk", _i32), ("q_rows", _vp), ("attn_scratch", _vp)]      # ABI 9: key-block attention


class _KState(ctypes.Structure):      # onebit_kshard_state_t (ABI 8; the attention fields: ABI 9)
    _fields_ = [("struct_size", ctypes.c_uint64), ("token", _vp), ("pos", _vp), ("out_tokens", _vp), ("max_out", _i32),
                ("hres0", _vp), ("hres1", _vp), ("x", _vp), ("u_q", _vp), ("u_k", _vp), ("u_v", _vp), ("attn_out", _vp),
                ("u_gate", _vp), ("u_up", _vp), ("act", _vp), ("u_down", _vp),
                ("z_qkv", _vp), ("z_o", _vp), ("z_gu", _vp), ("z_down", _vp),
                ("logits", _vp), ("part_val", _vp), ("part_idx", _vp), ("tile_stats", _vp),
                ("k0_hidden", _i32), ("k0_attn", _i32), ("k0_inter", _i32),
                ("attn_chunk", _i32), ("attn_splits", _i32), ("attn_scratch", _vp)]


KSEG_QKV, KSEG_ATTN_O, KSEG_GATE_UP, KSEG_DOWN, KSEG_HEAD = 0, 1, 2, 3, 4


class _Seg(ctypes.Structure):         # onebit_seg_t (ABI 9)
    _fields_ = [("row0", _i32), ("n", _i32), ("slot", _i32), ("past", _i32)]


class _MixedState(ctypes.Structure):  # onebit_mixed_state_t (ABI 9)
    _fields_ = [("struct_size", ctypes.c_uint64), ("n_rows", _i32), ("n_dec", _i32), ("n_seg", _i32), ("n_out", _i32),
                ("n_slots", _i32), ("attn_chunk", _i32), ("dec_ctx", _i32),
                ("tokens", _vp), ("row_slot", _vp), ("row_pos", _vp), ("segs", ctypes.POINTER(_Seg)), ("out_rows", _vp),
                ("next_tokens", _vp), ("logits", _vp), ("part_val", _vp), ("part_idx", _vp),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t)]


class _SpecState(ctypes.Structure):   # onebit_spec_state_t (additive to ABI 10)
    _fields_ = [("struct_size", ctypes.c_uint64), ("k", _i32), ("n_slots", _i32), ("attn_chunk", _i32), ("attn_splits", _i32),
                ("ngram_max", _i32), ("ngram_min", _i32),
                ("tokens", _vp), ("row_slot", _vp), ("row_pos", _vp), ("drafts", _vp), ("chosen", _vp), ("pos", _vp),
                ("remaining", _vp), ("history", _vp), ("record", _vp), ("logits", _vp), ("part_val", _vp), ("part_idx", _vp),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t)]


class _FusedIn(ctypes.Structure):
    _fields_ = [("xin", _vp), ("embed", _vp), ("hres_in", _vp), ("u_prev", _vp), ("rms_w", _vp),
                ("u_gate", _vp), ("u_up", _vp), ("token", _vp), ("hres_out", _vp),
                ("rms_eps", _f), ("ln_eps", _f), ("st_prev", _vp), ("st_gate", _vp), ("st_up", _vp),
                ("st_out", _vp * 3)]


PRO_PLAIN, PRO_EMBED_RMS, PRO_RES_LN_RMS, PRO_SWIGLU = 0, 1, 2, 3


def tile_stats_floats(n: int) -> int:
    """fp32 elements of the per-tile LayerNorm partials of an n-vector (whole blocks of 256 tiles)."""
    return ((n + 4095) // 4096) * 512


@functools.lru_cache(maxsize=None)
def _field_names(cls) -> frozenset:
    return frozenset(f[0] for f in cls._fields_)


def make_state(cls, tensors=None, **fields):
    """A struct of mirror ``cls`` -- or, given an instance, a copy of it -- with ``struct_size`` filled where the struct has one,
    ``tensors`` (field name -> tensor, None = a null pointer) stored as ``data_ptr()`` and ``fields`` stored by name.  A name the
    struct does not have raises AttributeError (a plain setattr on a ctypes Structure would create a Python attribute and leave
    the C field as it was)."""
    st = cls() if isinstance(cls, type) else type(cls).from_buffer_copy(cls)
    names = _field_names(type(st))
    if "struct_size" in names:
        st.struct_size = ctypes.sizeof(st)
    if tensors:
        fields.update((k, None if t is None else t.data_ptr()) for k, t in tensors.items())
    if not names.issuperset(fields):
        raise AttributeError(f"{type(st).__name__} has no field {sorted(set(fields) - names)}")
    for k, v in fields.items():
        setattr(st, k, v)
    return st


def _proj(m, allow_bias: bool = False, kslice=None) -> _Proj:
    """``onebit_proj_t`` of the BitLinearInf ``m`` (``kslice = (k0, k1)``: of its K slice, in place)."""
    if m.bias is not None and not allow_bias:
        raise ValueError(
            "the fused decode engines take a projection bias on q / k / v / o_proj only (config.attention_bias, "
            "modeling_bitllama.py:451-454: the reference's MLP projections have none); decode this checkpoint through the module "
            "path instead: model.generate(...) or ContinuousBatcher(..., native=False)")
    if m.bias is not None and (m.bias.dtype != torch.float16 or not m.bias.is_contiguous()):
        raise ValueError("the fused decode engines run fp16 parameters: pass the model through engine.fp16_view()")
    if m.weight_scale.dtype != torch.float16 or m.input_factor.dtype != torch.float16:
        raise ValueError("the fused decode engines run fp16 parameters: pass the model through engine.fp16_view()")
    if m.in_features % 32 != 0:
        raise ValueError(f"DecodeEngine: in_features={m.in_features} is not a multiple of 32; use the module path")
    w = m.weight
    if w.stride(1) != 1 or not m.weight_scale.is_contiguous() or not m.input_factor.is_contiguous():
        raise ValueError("DecodeEngine: parameters must be contiguous")
    # a K slice is a byte-column window of the packed matrix (the ABI takes the row pitch) and h[k0:k1]
    k0, k1 = kslice if kslice is not None else (0, m.in_features)
    return make_state(_Proj, weight=w.data_ptr() + k0 // 8, input_factor=m.input_factor.data_ptr() + 2 * k0,
                      weight_scale=m.weight_scale.data_ptr(), N=m.out_features, K=k1 - k0, ldw_bytes=w.stride(0))


def _model_struct(model, caches, max_len: int, krange=None):
    """ctypes image of ``onebit_model_t`` for ``model`` with per-layer (k, v) cache tensors; returns
    (struct, objects that must stay alive as long as the struct is used).  ``krange(K) -> (k0, k1)``: describe every
    projection's K SLICE instead (onebit_decode_step_ksharded: the rank's window into the full packed matrices)."""
    cfg = model.config
    dev, f16 = model.lm_head.weight.device, torch.float16
    cos, sin = model._rope_tables(dev, f16)
    cos, sin = cos.contiguous(), sin.contiguous()
    layers = (_Layer * cfg.num_hidden_layers)()
    for i, (layer, (kc, vc)) in enumerate(zip(model.model.layers, caches)):
        a, mlp = layer.self_attn, layer.mlp
        for w in (layer.input_layernorm.weight, layer.post_attention_layernorm.weight):
            if w.dtype != f16:
                raise ValueError("the decode steps need fp16 RMSNorm weights")
        qkv_b = [p.bias is not None for p in (a.q_proj, a.k_proj, a.v_proj)]
        if any(qkv_b) and not all(qkv_b):
            raise ValueError("the fused decode engines need a bias on all of q / k / v_proj or on none (config.attention_bias)")
        pr = lambda p, bias: _proj(p, bias, None if krange is None else krange(p.in_features))
        layers[i] = make_state(
            _Layer, dict(input_layernorm_w=layer.input_layernorm.weight, post_attention_layernorm_w=layer.post_attention_layernorm.weight,
                         k_cache=kc, v_cache=vc, q_bias=a.q_proj.bias, k_bias=a.k_proj.bias, v_bias=a.v_proj.bias, o_bias=a.o_proj.bias),
            q=pr(a.q_proj, True), k=pr(a.k_proj, True), v=pr(a.v_proj, True), o=pr(a.o_proj, True),
            gate=pr(mlp.gate_proj, False), up=pr(mlp.up_proj, False), down=pr(mlp.down_proj, False))
    m = make_state(_Model, dict(embed=model.model.embed_tokens.weight, final_norm_w=model.model.norm.weight, lm_head=model.lm_head.weight,
                                rope_cos=cos, rope_sin=sin),
                   n_layers=cfg.num_hidden_layers, hidden=cfg.hidden_size, intermediate=cfg.intermediate_size,
                   n_heads=cfg.num_attention_heads, n_kv_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, vocab=cfg.vocab_size,
                   max_len=max_len, rms_eps=cfg.rms_norm_eps, ln_eps=1e-5, layers=layers)
    return m, [layers, cos, sin]
