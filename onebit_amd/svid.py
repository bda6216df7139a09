"""SVID start checkpoints on MI355X: a full-precision LLaMA teacher -> the 1-bit student that KD training starts from.

The reference builds them on the CPU (``scripts/build_start_ckpt.py``): for every projection ``A`` [N, K] it fits
``sklearn.decomposition.NMF(n_components=1, init='random', random_state=0)`` to ``|A|`` and stores

    weight_scale = W[:, 0]   input_factor = H[0]   weight = sign(A) * 0.01            (``:30-34``)

For one component sklearn's coordinate-descent solver is plain alternating least squares, started from draws of
``numpy.random.RandomState(0)`` that fix how the scale is split between the two vectors:

    avg = sqrt(mean(X));  h = |avg * randn(1, K)|  (drawn first);  w = |avg * randn(N, 1)|
    repeat:  w = max(X h / h.h, 0);  h = max(X^T w / w.w, 0)
    until the summed projected-gradient violation falls to tol = 1e-4 of the first iteration's (max_iter = 200)

``svid_init`` makes those draws on the host (K + N numbers, no sklearn needed); the iterations and the sign / pack / residual
pass are HIP kernels behind the C ABI (``onebit_svid_*``, ``csrc/ob_svid.h``): fp32 arithmetic on the fp16 or fp32 matrix,
``|A|`` never materialised, sums in a fixed order (bit-reproducible).  One iteration is three launches on the one-pass route
(the pass over ``A``, the column finalize, the statistics) and four on the two-pass route.  The host reads the violation (one
float) back per iteration to apply the stopping rule -- this is an offline tool, not a path to capture in a graph.
``mean(|A|)`` for the draws comes from torch: float32 row sums of ``|A|`` reduced straight from the stored dtype (one more
read of ``A``, [N] floats out, no copy of the matrix), added up in float64.  There is no CPU fallback: CPU tensors raise.

    python -m onebit_amd.svid TEACHER_DIR OUT_DIR [--packed]
"""
from __future__ import annotations

import json
import math
import os
import re
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .bitnet import _dtype_code, _require_gpu, _stream_ptr

__all__ = ["SvidResult", "SvidWork", "svid_init", "svid_decompose", "svid_start_layer", "build_start_state_dict", "build_inference_state_dict"]

SvidResult = namedtuple("SvidResult", ["weight_scale", "input_factor", "n_iter", "rel_residual"])

_PROJ_KEY = re.compile(r"^model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)\.weight$")


def svid_init(N: int, K: int, mean, dtype, random_state: int = 0):
    """``(w0 [N], h0 [K])``: sklearn's ``init='random'`` draws for one component on a matrix of that shape, mean and dtype.

    ``dtype`` is the dtype sklearn computes in: float32 for a float32 matrix (the draws are rounded to float32 before the
    product and the ``abs``), float64 for anything else (``check_array`` promotes float16).  ``H`` is drawn before ``W``."""
    ct = np.float32 if np.dtype(dtype) == np.float32 else np.float64
    avg = np.sqrt(np.asarray(mean, dtype=ct))
    rng = np.random.RandomState(random_state)
    h = avg * rng.standard_normal(size=(1, K)).astype(ct, copy=False)
    w = avg * rng.standard_normal(size=(N, 1)).astype(ct, copy=False)
    return np.abs(w)[:, 0], np.abs(h)[0]


def _matrix(weight: torch.Tensor, what: str):
    _require_gpu(weight, what)
    if weight.dim() != 2:
        raise ValueError(f"{what}: expected a 2-D weight [N, K], got {tuple(weight.shape)}")
    N, K = weight.shape
    if N < 1 or K < 1 or K % 8 != 0:
        raise ValueError(f"{what}: in_features={K} must be a positive multiple of 8 (and out_features={N} >= 1)")
    if weight.dtype not in (torch.float16, torch.float32):
        weight = weight.float()
    # a row-strided view of a wider buffer is read in place when its rows keep 16-byte chunks aligned
    if weight.stride(1) != 1 or weight.stride(0) < K or weight.stride(0) % 8 != 0 or weight.data_ptr() % 16 != 0:
        weight = weight.contiguous()
    return weight, N, K


class SvidWork:
    """The device buffers of one matrix ``a`` [N, K] (as ``svid_decompose`` passes it on: float16 or float32, unit column
    stride, 16-byte aligned rows) -- the statistics, the residual sums and the workspace -- and the two C-ABI calls on them.
    ``iterate`` updates float32 ``w`` [N] and ``h`` [K] in place; ``emit`` fills the outputs it is given."""

    def __init__(self, a: torch.Tensor, N: int, K: int):
        self.lib = _lib.load()
        self.a, self.N, self.K, self.dev = a, N, K, a.device
        self.code = _dtype_code(a.dtype)
        self.nws = self.lib.onebit_svid_workspace_bytes(N, K, self.code)
        self.ws = torch.empty(max(self.nws, 16), dtype=torch.uint8, device=self.dev)
        self.stats = torch.zeros(_lib.SVID_STATS, dtype=torch.float32, device=self.dev)
        self.sums = torch.zeros(2, dtype=torch.float32, device=self.dev)

    def iterate(self, w, h, route):
        with torch.cuda.device(self.dev):
            rc = self.lib.onebit_svid_iterate(self.a.data_ptr(), self.code, self.a.stride(0), w.data_ptr(), h.data_ptr(), self.stats.data_ptr(),
                                              self.ws.data_ptr(), self.nws, self.N, self.K, route, _stream_ptr(self.dev))
        _lib.check(rc, "onebit_svid_iterate")

    def emit(self, w, h, latent=None, scale=0.01, packed=None, sums=True):
        with torch.cuda.device(self.dev):
            rc = self.lib.onebit_svid_emit(self.a.data_ptr(), self.code, self.a.stride(0), w.data_ptr(), h.data_ptr(),
                                           None if latent is None else latent.data_ptr(), 0 if latent is None else _dtype_code(latent.dtype),
                                           scale, None if packed is None else packed.data_ptr(), self.sums.data_ptr() if sums else None,
                                           self.ws.data_ptr(), self.nws, self.N, self.K, _stream_ptr(self.dev))
        _lib.check(rc, "onebit_svid_emit")

    def rel_residual(self) -> float:
        s0, s1 = self.sums.tolist()
        return math.sqrt(s0 / s1) if s1 > 0 else 0.0


def _fit(wk: SvidWork, tol, max_iter, n_iter, random_state, route):
    """the alternating iterations on wk.a; returns (w, h, iterations run)"""
    a, N, K = wk.a, wk.N, wk.K
    # sum |a|: float32 row sums reduced from the stored dtype (float16 -> float32 and float32 -> float32 are torch's fused
    # reductions: no copy of the matrix, [N] floats out), added up in float64
    total = float(torch.linalg.vector_norm(a, ord=1, dim=1, dtype=torch.float32).double().sum())
    if not math.isfinite(total):
        raise ValueError("svid: the weight contains NaN or infinity (or its sums overflow float32)")
    # the mean in the dtype sklearn would hold it in: float32 for a float32 matrix, float64 after its promotion of float16
    ct = np.float32 if a.dtype == torch.float32 else np.float64
    w0, h0 = svid_init(N, K, ct(total / (N * K)), ct, random_state)
    w = torch.from_numpy(w0.astype(np.float32)).to(wk.dev)
    h = torch.from_numpy(h0.astype(np.float32)).to(wk.dev)
    fixed = n_iter is not None
    limit = int(n_iter) if fixed else int(max_iter)
    if limit < 1:
        raise ValueError("svid: at least one iteration")
    viol0, it = None, 0
    while it < limit:
        wk.iterate(w, h, route)
        it += 1
        if fixed and it > 1:
            continue                                      # a fixed count needs the read-back only once, for the finiteness check
        viol = float(wk.stats[0])
        if not math.isfinite(viol):                       # the kernels' own sums: a product with h may overflow where the row sums did not
            raise ValueError("svid: the weight contains NaN or infinity (or its sums overflow float32)")
        if it == 1:
            viol0 = viol
        if not fixed and (viol0 == 0.0 or viol / viol0 <= tol):
            break
    return w, h, it


def svid_decompose(weight: torch.Tensor, tol: float = 1e-4, max_iter: int = 200, n_iter=None, random_state: int = 0, route: int = 0,
                   dtype=None) -> SvidResult:
    """``weight_scale`` [N], ``input_factor`` [K] of a teacher projection ``weight`` [N, K] (float16 or float32, on the GPU).

    ``n_iter=None`` applies the reference's stopping rule (``tol``, ``max_iter`` are sklearn's defaults), an integer runs exactly
    that many iterations.  ``route`` 0 picks the kernel route, 1 / 2 force the one-pass / two-pass route.  The vectors are
    float32 (what the reference gets for a float32 teacher) unless ``dtype`` casts them.  ``rel_residual`` is
    ``sqrt(sum (|a| - w_i h_j)^2 / sum a^2)``: ``|A - sign(A) * (w h^T)|_F / |A|_F`` away from exact zeros.
    Non-finite input raises ``ValueError``."""
    a, N, K = _matrix(weight, "svid_decompose")
    wk = SvidWork(a, N, K)
    w, h, it = _fit(wk, tol, max_iter, n_iter, random_state, route)
    wk.emit(w, h)
    rel = wk.rel_residual()
    if dtype is not None:
        w, h = w.to(dtype), h.to(dtype)
    return SvidResult(w, h, it, rel)


def svid_start_layer(weight: torch.Tensor, latent_dtype=None, scale: float = 0.01):
    """``(latent_weight, weight_scale, input_factor)`` of one projection: ``build_start_ckpt.py:30-34``.  ``latent_weight`` is
    ``sign(weight) * scale`` in ``latent_dtype`` (default: the weight's), the vectors are float32."""
    a, N, K = _matrix(weight, "svid_start_layer")
    wk = SvidWork(a, N, K)
    w, h, _ = _fit(wk, 1e-4, 200, None, 0, 0)
    latent = torch.empty((N, K), dtype=latent_dtype or a.dtype, device=a.device)
    wk.emit(w, h, latent=latent, scale=scale, sums=False)
    return latent, w, h


def _build(teacher_sd, device, progress, packed: bool):
    out = {}
    todo = [k for k, v in teacher_sd.items() if _PROJ_KEY.match(k) and v.dim() == 2 and v.is_floating_point()]
    done = 0
    for k, v in teacher_sd.items():
        if k not in todo:
            out[k] = v
            continue
        stem = k[:-len(".weight")]
        a, N, K = _matrix(v.to(device), stem)
        wk = SvidWork(a, N, K)
        w, h, it = _fit(wk, 1e-4, 200, None, 0, 0)
        if packed:
            body = torch.empty((N, K // 8), dtype=torch.int8, device=a.device)
            wk.emit(w, h, packed=body)
        else:
            body = torch.empty((N, K), dtype=a.dtype, device=a.device)
            wk.emit(w, h, latent=body)
        # one dtype per layer, as BitLinear needs: float32 vectors for a float32 teacher (the reference's), float16 for a float16 one
        out[k] = body.cpu()
        out[stem + ".weight_scale"] = w.to(a.dtype).cpu()
        out[stem + ".input_factor"] = h.to(a.dtype).cpu()
        done += 1
        if progress is not None:
            progress(done, len(todo), stem, it, wk.rel_residual())
    return out


def build_start_state_dict(teacher_sd, device="cuda", progress=None):
    """A LLaMA teacher's state dict -> the student's start checkpoint: every ``model.layers.{i}.{self_attn.{q,k,v,o}_proj |
    mlp.{gate,up,down}_proj}.weight`` becomes ``weight`` (latent, ``sign * 0.01``), ``weight_scale`` and ``input_factor`` --
    ``train.BitLinear``'s keys; everything else is copied untouched.  ``progress(done, total, name, n_iter, rel_residual)``."""
    return _build(teacher_sd, device, progress, packed=False)


def build_inference_state_dict(teacher_sd, device="cuda", progress=None):
    """The same vectors with the signs packed directly (int8 [N, K / 8]; no [N, K] latent tensor is formed): bit-identical to
    ``checkpoint.convert_train_state_dict(build_start_state_dict(teacher_sd))``."""
    return _build(teacher_sd, device, progress, packed=True)


def main(argv=None):
    import argparse
    from .checkpoint import WEIGHTS_NAME, write_checkpoint
    ap = argparse.ArgumentParser(prog="python -m onebit_amd.svid", description="teacher checkpoint -> 1-bit start checkpoint (SVID)")
    ap.add_argument("teacher_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--packed", action="store_true", help="write packed inference weights instead of latent training weights")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    with open(os.path.join(args.teacher_dir, "config.json")) as f:
        cfg = json.load(f)
    sd = torch.load(os.path.join(args.teacher_dir, WEIGHTS_NAME), map_location="cpu", weights_only=True)
    report = lambda i, n, name, it, rel: print(f"[{i}/{n}] {name}: {it} iterations, relative residual {rel:.4f}", flush=True)
    out = (build_inference_state_dict if args.packed else build_start_state_dict)(sd, args.device, report)
    cfg.update(model_type="bitllama", architectures=["BitLlamaForCausalLMInf" if args.packed else "BitLlamaForCausalLM"])
    write_checkpoint(args.out_dir, cfg, out)


if __name__ == "__main__":
    main()
