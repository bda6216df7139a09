"""The train-mode model and eager causal attention, restated on torch ops -- helper of tests/test_train_model_cpu.py,
tests/test_gpu_train_attention.py and tests/test_gpu_train_model.py.  TEST INFRASTRUCTURE: only tests import it.

Written from the arithmetic of the reference's ``BitLlamaForCausalLM`` (module names as there, so the state-dict keys are its
keys), on ``oracle.train_ref.BitLinear``.  Every op runs in the dtype it is given -- float64 (the truth), float32, or float16 on
the CPU (the restatement's own rounding, which sets the bars: ``_train_ref.MARGIN x`` its distance to the truth, per tensor, in
``_train_ref``'s two metrics).  Where the reference upcasts to float32 (RMSNorm, the softmax, the logits) a float64 evaluation
stays float64.  Pinned by tests/golden/train_model_tiny.npz (tests/golden/gen_goldens_train_model.py records it from the reference
class; tests/test_train_model_cpu.py compares).

The parameters of the fixture are not stored (1.6 MB in fp32): ``make_params(cfg, seed)`` regenerates them from numpy's frozen
``RandomState`` stream, rounded to float16 so that every dtype sees the same values.
"""
import functools
import math
import os

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

from oracle.train_ref import BitLinear

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_model_tiny.npz")
RECORDS = ("mha", "gqa")
CONFIGS = {
    "mha": dict(vocab_size=320, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                num_key_value_heads=2, max_position_embeddings=64),
    "gqa": dict(vocab_size=320, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                num_key_value_heads=1, max_position_embeddings=64),
}
SEEDS = {"mha": 4101, "gqa": 4102}
BATCH, SEQ = 2, 24
# the parameters whose gradients the fixture records
GRAD_KEYS = ("model.embed_tokens.weight", "lm_head.weight",
             "model.layers.0.self_attn.q_proj.weight", "model.layers.0.self_attn.q_proj.weight_scale",
             "model.layers.0.self_attn.q_proj.input_factor",
             "model.layers.1.mlp.down_proj.weight", "model.layers.1.mlp.down_proj.weight_scale",
             "model.layers.1.mlp.down_proj.input_factor")


def _wide(dtype):
    return torch.float64 if dtype == torch.float64 else torch.float32


# ---------------------------------------------------------------------------------------------------------------- attention --
def ref_attention(q, k, v):
    """Eager causal attention of token-major q [B, S, H, D], k / v [B, S, Hkv, D] -> [B, S, H, D]: scores = q k^T / sqrt(D) in the
    tensor dtype, plus the dtype's most negative number above the diagonal, softmax in float32 (float64 for float64), the
    probabilities back in the tensor dtype, times v."""
    B, S, H, D = q.shape
    rep = H // k.shape[2]
    qt = q.permute(0, 2, 1, 3)
    kt = k.permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    vt = v.permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    scores = torch.matmul(qt, kt.transpose(-1, -2)) / math.sqrt(D)
    above = torch.ones(S, S, dtype=torch.bool).triu(1)
    scores = scores + torch.zeros(S, S, dtype=q.dtype).masked_fill(above, torch.finfo(q.dtype).min)
    p = F.softmax(scores, dim=-1, dtype=_wide(q.dtype)).to(q.dtype)
    return torch.matmul(p, vt).permute(0, 2, 1, 3).contiguous()


def ref_lse(q, k):
    """log sum_j<=i exp(q_i k_j / sqrt(D)) -> [B, H, S] in the wide dtype (the scores themselves in the tensor dtype, as above)"""
    B, S, H, D = q.shape
    rep = H // k.shape[2]
    scores = torch.matmul(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3).repeat_interleave(rep, dim=1).transpose(-1, -2)) / math.sqrt(D)
    scores = scores.to(_wide(q.dtype)).masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    return torch.logsumexp(scores, dim=-1)


def attention_case(B, S, H, Hkv, D, seed, kind="random"):
    """q, k, v, dO as float64 tensors of float16-representable values.  kind "spread": scores of one row span far more than 8 log2
    units -- an early key, a middle key and a late key far above the rest, each above the one before."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).half().double()
    q, k, v, d_o = r(B, S, H, D), r(B, S, Hkv, D), r(B, S, Hkv, D), r(B, S, H, D)
    if kind == "spread":
        # every query leans along u (q . u / sqrt(D) ~ 1.5 sqrt(D)); keys 1, 70 and S - 3 are 0.5 u, 0.75 u and 1.5 u: scores of about
        # 6 / 9 / 18 at D = 64 (8.5 / 12.7 / 25.5 at D = 128) over a background of +-0.4 -- steps of ~4-6 and ~13-18 log2 units
        assert S > 80
        u = torch.sign(torch.randn(D, generator=g)).double()
        q = (0.25 * q + 1.5 * u).half().double()
        k = (0.25 * k).half().double()
        k[:, 1], k[:, 70], k[:, S - 3] = 0.5 * u, 0.75 * u, 1.5 * u
    return {"q": q, "k": k, "v": v, "d_o": d_o}


def run_attention(case, dtype, fn=ref_attention, device="cpu", lse_fn=None):
    """o, dq, dk, dv (and lse) of `fn` on `case` in `dtype` as float64 CPU tensors; loss = (o * dO).sum()."""
    q, k, v = (case[n].to(dtype).to(device).clone().requires_grad_(True) for n in ("q", "k", "v"))
    d_o = case["d_o"].to(dtype).to(device)
    out = fn(q, k, v)
    lse = None
    if isinstance(out, tuple):
        out, lse = out
    elif lse_fn is not None:
        lse = lse_fn(q.detach(), k.detach())
    out.backward(d_o)
    res = {"o": out.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
    if lse is not None:
        res["lse"] = lse.detach()
    return {n: t.double().cpu() for n, t in res.items()}


# -------------------------------------------------------------------------------------------------------------------- model --
class RMSNorm(nn.Module):
    def __init__(self, n, eps, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(n, dtype=dtype), requires_grad=False)
        self.eps = eps

    def forward(self, x):
        xw = x.to(_wide(x.dtype))
        xw = xw * torch.rsqrt(xw.pow(2).mean(-1, keepdim=True) + self.eps)
        return self.weight * xw.to(x.dtype)


def rope(x, cos, sin):
    """x [B, S, heads, D]: x cos + (-x2 | x1) sin with the halves x1 | x2 of the last axis"""
    h = x.shape[-1] // 2
    rot = torch.cat((-x[..., h:], x[..., :h]), dim=-1)
    return x * cos[None, :, None, :] + rot * sin[None, :, None, :]


def rope_ref_tables(D, S, theta, dtype):
    """cos / sin of position * theta^(-2 i / D), computed in float32 (they are the model's constants), cast to `dtype`"""
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.outer(torch.arange(S, dtype=torch.float32), inv)
    ang = torch.cat((ang, ang), dim=-1)
    return ang.cos().to(dtype), ang.sin().to(dtype)


class _MLP(nn.Module):
    def __init__(self, cfg, dtype):
        super().__init__()
        Hd, I = cfg["hidden_size"], cfg["intermediate_size"]
        self.gate_proj, self.up_proj, self.down_proj = BitLinear(Hd, I, dtype=dtype), BitLinear(Hd, I, dtype=dtype), BitLinear(I, Hd, dtype=dtype)

    def forward(self, x):
        return self.down_proj(F.silu(self.gate_proj(x)) * self.up_proj(x))


class _Attention(nn.Module):
    def __init__(self, cfg, dtype):
        super().__init__()
        Hd, H, Hkv = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"]
        self.H, self.Hkv, self.D = H, Hkv, Hd // H
        bias = bool(cfg.get("attention_bias", False))
        self.q_proj = BitLinear(Hd, H * self.D, bias=bias, dtype=dtype)
        self.k_proj = BitLinear(Hd, Hkv * self.D, bias=bias, dtype=dtype)
        self.v_proj = BitLinear(Hd, Hkv * self.D, bias=bias, dtype=dtype)
        self.o_proj = BitLinear(H * self.D, Hd, bias=bias, dtype=dtype)

    def forward(self, x, cos, sin):
        B, S, Hd = x.shape
        x2 = x.reshape(B * S, Hd)
        q = rope(self.q_proj(x2).view(B, S, self.H, self.D), cos, sin)
        k = rope(self.k_proj(x2).view(B, S, self.Hkv, self.D), cos, sin)
        v = self.v_proj(x2).view(B, S, self.Hkv, self.D)
        return self.o_proj(ref_attention(q, k, v).reshape(B * S, self.H * self.D)).view(B, S, Hd)


class _Layer(nn.Module):
    def __init__(self, cfg, dtype):
        super().__init__()
        self.self_attn, self.mlp = _Attention(cfg, dtype), _MLP(cfg, dtype)
        eps = cfg.get("rms_norm_eps", 1e-6)
        self.input_layernorm, self.post_attention_layernorm = RMSNorm(cfg["hidden_size"], eps, dtype), RMSNorm(cfg["hidden_size"], eps, dtype)

    def forward(self, h, cos, sin):
        h = h + self.self_attn(self.input_layernorm(h), cos, sin)
        B, S, Hd = h.shape
        return h + self.mlp(self.post_attention_layernorm(h).reshape(B * S, Hd)).view(B, S, Hd)


class _Body(nn.Module):
    def __init__(self, cfg, dtype):
        super().__init__()
        self.embed_tokens = nn.Embedding(cfg["vocab_size"], cfg["hidden_size"], dtype=dtype)
        self.layers = nn.ModuleList([_Layer(cfg, dtype) for _ in range(cfg["num_hidden_layers"])])
        self.norm = RMSNorm(cfg["hidden_size"], cfg.get("rms_norm_eps", 1e-6), dtype)


class RefTrainModel(nn.Module):
    """forward(input_ids, labels) -> (logits in the wide dtype, the L + 1 hidden states, the shifted cross-entropy or None)"""

    def __init__(self, cfg, dtype):
        super().__init__()
        self.cfg, self.dtype = cfg, dtype
        self.model = _Body(cfg, dtype)
        self.lm_head = nn.Linear(cfg["hidden_size"], cfg["vocab_size"], bias=False, dtype=dtype)

    def forward(self, input_ids, labels=None, output_hidden_states=True):
        cfg = self.cfg
        cos, sin = rope_ref_tables(cfg["hidden_size"] // cfg["num_attention_heads"], input_ids.shape[1], cfg.get("rope_theta", 10000.0), self.dtype)
        h = self.model.embed_tokens(input_ids)
        states = []
        for layer in self.model.layers:
            states.append(h)
            h = layer(h, cos, sin)
        h = self.model.norm(h)
        states.append(h)
        logits = self.lm_head(h).to(_wide(self.dtype))
        loss = None
        if labels is not None:
            V = logits.shape[-1]
            loss = F.cross_entropy(logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100)
        return logits, tuple(states), loss


# ------------------------------------------------------------------------------------------------------------------ fixture --
def proj_shapes(cfg):
    Hd, I, H, Hkv = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"]
    D = Hd // H
    return [("self_attn.q_proj", Hd, H * D), ("self_attn.k_proj", Hd, Hkv * D), ("self_attn.v_proj", Hd, Hkv * D),
            ("self_attn.o_proj", H * D, Hd), ("mlp.gate_proj", Hd, I), ("mlp.up_proj", Hd, I), ("mlp.down_proj", I, Hd)]


def make_params(cfg, seed):
    """The fixture's state dict as float32 tensors of float16-representable values, from numpy's frozen RandomState stream.
    Latent weights +-(0.05 .. 0.35): away from zero, so sign() is the same in every precision; weight_scale and input_factor
    0.05 .. 0.15 with a fifth of the signs flipped."""
    rs = np.random.RandomState(seed)
    h16 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float32))

    def vec(n):
        return h16(0.1 * (0.5 + rs.rand(n)) * np.where(rs.rand(n) < 0.2, -1.0, 1.0))
    sd = {}
    Hd = cfg["hidden_size"]
    for l in range(cfg["num_hidden_layers"]):
        for name, K, N in proj_shapes(cfg):
            pre = f"model.layers.{l}.{name}."
            sd[pre + "weight"] = h16((0.05 + 0.3 * rs.rand(N, K)) * np.where(rs.rand(N, K) < 0.5, -1.0, 1.0))
            sd[pre + "weight_scale"] = vec(N)
            sd[pre + "input_factor"] = vec(K)
        sd[f"model.layers.{l}.input_layernorm.weight"] = torch.ones(Hd)
        sd[f"model.layers.{l}.post_attention_layernorm.weight"] = torch.ones(Hd)
    sd["model.embed_tokens.weight"] = h16(rs.randn(cfg["vocab_size"], Hd))
    sd["model.norm.weight"] = torch.ones(Hd)
    sd["lm_head.weight"] = h16(0.05 * rs.randn(cfg["vocab_size"], Hd))
    return sd


def make_batch(cfg, seed):
    rs = np.random.RandomState(seed + 50000)
    ids = rs.randint(0, cfg["vocab_size"], size=(BATCH, SEQ)).astype(np.int64)
    labels = ids.copy()
    labels[0, :5] = -100            # a masked prompt
    labels[1, 9] = labels[1, 17] = -100
    return torch.from_numpy(ids), torch.from_numpy(labels)


@functools.lru_cache(maxsize=None)
def golden(record):
    """{name: numpy array} of one record of the fixture (names without the record prefix)"""
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k[len(record) + 1:]: z[k] for k in z.files if k.startswith(record + "/")}


def names_of(cfg):
    """what a run records: logits, hidden_0 .. hidden_L, loss, grad/<key> for GRAD_KEYS"""
    return ["logits"] + [f"hidden_{i}" for i in range(cfg["num_hidden_layers"] + 1)] + ["loss"] + ["grad/" + k for k in GRAD_KEYS]


def run_model(model, sd, input_ids, labels, dtype, device="cpu", trainable_extra=("model.embed_tokens.weight", "lm_head.weight")):
    """Load `sd` into `model` (already built for `dtype`), move to `device`, run forward with labels and hidden states and one
    backward of the loss -> {name: float64 CPU tensor} over names_of.  The embedding and lm_head are made trainable for the
    run (the reference freezes them; the fixture records their gradients all the same)."""
    model.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    model = model.to(device)
    params = dict(model.named_parameters())
    for k in trainable_extra:
        params[k].requires_grad_(True)
    for p in params.values():
        p.grad = None
    out = model(input_ids.to(device), labels=labels.to(device), output_hidden_states=True)
    logits, states, loss = out[0], out[1], out[2]
    loss.backward()
    res = {"logits": logits, "loss": loss}
    for i, s in enumerate(states):
        res[f"hidden_{i}"] = s
    for k in GRAD_KEYS:
        assert params[k].grad is not None, k
        res["grad/" + k] = params[k].grad
    return {n: t.detach().double().cpu() for n, t in res.items()}


_REF = {}


def reference(record, dtype):
    """the restatement on the CPU in `dtype` on the fixture's parameters and batch; evaluated once and kept: do not modify"""
    key = (record, str(dtype))
    if key not in _REF:
        cfg = CONFIGS[record]
        ids, labels = make_batch(cfg, SEEDS[record])
        _REF[key] = run_model(RefTrainModel(cfg, dtype), make_params(cfg, SEEDS[record]), ids, labels, dtype)
    return _REF[key]
