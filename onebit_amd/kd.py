"""Knowledge-distillation loss for 1-bit LLaMA training on MI355X: the objective ``train.BitLinear`` is trained against.

``KDLoss`` reproduces the reference's ``KDTrainer.compute_loss`` (``llama_factory/llamafactory/kd.py:34-113``) on logits and
hidden states that the caller's teacher and student models produced:

    loss = kd_alpha * kd_loss_scale * KL + (1 - kd_alpha) * CE + kd_beta * sum_i mean_rows |t^_i - s^_i|^2

* ``KL`` is ``F.kl_div(log_softmax(student), softmax(teacher), reduction="batchmean")`` on ``[B, S, V]`` logits: the sum over
  ALL rows divided by ``B`` -- not by ``B * S`` (``:36-39``; batchmean divides by ``input.size(0)``).
* ``CE`` is the student's causal-LM loss: row ``(b, s)`` against ``labels[b, s + 1]``, mean over the labelled rows, NaN when
  there are none (and then ``(1 - kd_alpha) * CE`` is NaN even for ``kd_alpha = 1``, as in the reference).
* the hidden-state term runs over entries ``0 .. n_layers - 1`` of the hidden-state tuples (``:87-96``): the embedding output
  and every layer's output but the last one's, which therefore gets no gradient from it.
* the attention-weight term (``kd_gamma``, ``:100-111``) needs materialised ``[B, H, S, S]`` attention weights, which this
  project's attention never forms; the shipped training scripts leave it at 0 and it raises ``NotImplementedError`` here.

Forward and backward are hand-written HIP kernels behind the C ABI (``onebit_kd_*``, ``csrc/ob_kd.h``): one read of each
operand per pass, no ``[T, V]`` temporaries besides the gradient itself, no atomics (bit-reproducible), the upstream gradient
folded in on the device.  There is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from .bitnet import _dtype_code, _require_gpu, _stream_ptr

__all__ = ["KDLoss", "kd_token_loss", "kd_hidden_loss"]


def _rows(x: torch.Tensor, what: str):
    _require_gpu(x, what)
    if x.dim() < 1 or x.shape[-1] == 0:
        raise ValueError(f"{what}: expected [..., width] with width > 0, got {tuple(x.shape)}")
    return x.reshape(-1, x.shape[-1]).contiguous()


class _KDTokenFn(torch.autograd.Function):
    """(loss, KL, CE) from [T, V] logits rows and per-row labels; w_kl / w_ce: the weights of sum(kl_row) and of mean(ce_row)."""

    @staticmethod
    def forward(ctx, s2, t2, row_labels, w_kl, w_ce, ignore_index):
        T, V = s2.shape
        code = _dtype_code(s2.dtype)
        dev = s2.device
        stats = torch.empty((T, _lib.KD_TOKEN_STATS), dtype=torch.float32, device=dev)
        sums = torch.zeros(3, dtype=torch.float32, device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            rc = lib.onebit_kd_token_forward(s2.data_ptr(), t2.data_ptr() if w_kl != 0.0 else None, None if row_labels is None else row_labels.data_ptr(),
                                             stats.data_ptr(), sums.data_ptr(), T, V, code, ignore_index, _stream_ptr(dev))
        _lib.check(rc, "onebit_kd_token_forward")
        kl_sum = sums[0].clone()                                             # clones: the caller's scalars do not alias what backward reads
        ce = sums[1] / sums[2] if row_labels is not None else None          # 0 / 0 = NaN without labelled rows, as torch's mean
        loss = kl_sum * w_kl if w_kl != 0.0 else torch.zeros((), dtype=torch.float32, device=dev)
        if ce is not None:
            loss = loss + w_ce * ce
        ctx.save_for_backward(s2, t2, row_labels, stats, sums)
        ctx.w_kl, ctx.w_ce, ctx.ignore_index, ctx.code = w_kl, w_ce, ignore_index, code
        ce_out = ce.clone() if ce is not None else torch.zeros((), dtype=torch.float32, device=dev)
        ctx.mark_non_differentiable(kl_sum, ce_out)
        return loss, kl_sum, ce_out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_kl, _g_ce):
        s2, t2, row_labels, stats, sums = ctx.saved_tensors
        T, V = s2.shape
        dev = s2.device
        g = g_loss.to(torch.float32).reshape(())
        c_ce = g * ctx.w_ce / sums[2] if row_labels is not None else torch.zeros_like(g)
        coef = torch.stack([g * ctx.w_kl, c_ce]).contiguous()               # stays on the device: no host sync
        grad = torch.empty_like(s2)
        lib = _lib.load()
        with torch.cuda.device(dev):
            rc = lib.onebit_kd_token_backward(s2.data_ptr(), t2.data_ptr() if ctx.w_kl != 0.0 else None, None if row_labels is None else row_labels.data_ptr(),
                                              stats.data_ptr(), coef.data_ptr(), grad.data_ptr(), T, V, ctx.code, ctx.ignore_index,
                                              _stream_ptr(dev))
        _lib.check(rc, "onebit_kd_token_backward")
        return grad, None, None, None, None, None


def kd_token_loss(student_logits, teacher_logits, labels=None, *, kd_alpha, kd_loss_scale, ignore_index=-100):
    """``(loss, kl, ce)`` with ``loss = kd_alpha * kd_loss_scale * KL + (1 - kd_alpha) * CE`` (fp32 scalars on the device).

    ``loss`` is differentiable w.r.t. ``student_logits`` (gradient in their dtype); ``kl`` (batchmean) and ``ce`` are detached.
    ``kd_loss_scale <= 0`` skips the KL term (``kd.py:73``), ``labels=None`` the CE term."""
    _require_gpu(student_logits, "kd_token_loss")
    _require_gpu(teacher_logits, "kd_token_loss (teacher)")
    if student_logits.dim() != 3 or student_logits.shape != teacher_logits.shape:
        raise ValueError(f"kd_token_loss: expected two [B, S, V] tensors, got {tuple(student_logits.shape)} and {tuple(teacher_logits.shape)}")
    if student_logits.dtype != teacher_logits.dtype:
        raise RuntimeError("kd_token_loss: student and teacher logits must share one dtype (float16 or float32)")
    B, S, V = student_logits.shape
    if B == 0 or S == 0:
        raise ValueError("kd_token_loss: empty batch")
    row_labels = None
    if labels is not None:
        _require_gpu(labels, "kd_token_loss (labels)")
        if labels.shape != (B, S):
            raise ValueError(f"kd_token_loss: labels must be [B, S] = {(B, S)}, got {tuple(labels.shape)}")
        # the causal shift: row (b, s) is scored against labels[b, s + 1], the last position of a sequence against nothing
        row_labels = torch.full((B, S), ignore_index, dtype=torch.int64, device=student_logits.device)
        row_labels[:, :-1] = labels[:, 1:]
        row_labels = row_labels.reshape(-1)
    use_kl = kd_loss_scale > 0.0
    w_kl = float(kd_alpha) * float(kd_loss_scale) / B if use_kl else 0.0
    loss, kl_sum, ce = _KDTokenFn.apply(_rows(student_logits, "kd_token_loss"), _rows(teacher_logits.detach(), "kd_token_loss"),
                                        row_labels, w_kl, 1.0 - float(kd_alpha), int(ignore_index))
    kl = kl_sum / B if use_kl else torch.zeros_like(kl_sum)
    return loss, kl, ce


class _KDHiddenFn(torch.autograd.Function):
    """mean over the rows of |t / max(|t|, eps) - s / max(|s|, eps)|^2 for one pair of [T, H] states."""

    @staticmethod
    def forward(ctx, s2, t2):
        T, H = s2.shape
        code = _dtype_code(s2.dtype)
        dev = s2.device
        stats = torch.empty((T, _lib.KD_HIDDEN_STATS), dtype=torch.float32, device=dev)
        sums = torch.zeros(3, dtype=torch.float32, device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            rc = lib.onebit_kd_hidden_forward(s2.data_ptr(), t2.data_ptr(), stats.data_ptr(), sums.data_ptr(), T, H, code, _stream_ptr(dev))
        _lib.check(rc, "onebit_kd_hidden_forward")
        ctx.save_for_backward(s2, t2, stats)
        ctx.code = code
        return sums[0] / T

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        s2, t2, stats = ctx.saved_tensors
        T, H = s2.shape
        dev = s2.device
        coef = (g.to(torch.float32).reshape(1) / T).contiguous()
        grad = torch.empty_like(s2)
        lib = _lib.load()
        with torch.cuda.device(dev):
            rc = lib.onebit_kd_hidden_backward(s2.data_ptr(), t2.data_ptr(), stats.data_ptr(), coef.data_ptr(), grad.data_ptr(), T, H,
                                               ctx.code, _stream_ptr(dev))
        _lib.check(rc, "onebit_kd_hidden_backward")
        return grad, None


def kd_hidden_loss(student_states, teacher_states):
    """``sum_i mean_rows |normalize(t_i) - normalize(s_i)|^2`` over the paired sequences of ``[..., H]`` states (fp32 scalar),
    differentiable w.r.t. every student tensor."""
    student_states, teacher_states = list(student_states), list(teacher_states)
    if len(student_states) != len(teacher_states) or not student_states:
        raise ValueError("kd_hidden_loss: expected two equally long, non-empty sequences of hidden states")
    total = None
    for s, t in zip(student_states, teacher_states):
        _require_gpu(s, "kd_hidden_loss")
        _require_gpu(t, "kd_hidden_loss (teacher)")
        if s.dtype != t.dtype:
            raise RuntimeError("kd_hidden_loss: student and teacher states must share one dtype (float16 or float32)")
        t2 = _rows(t.detach(), "kd_hidden_loss")
        s2 = s.reshape(-1, t2.shape[-1]).contiguous()                    # the reference views the student by the teacher's width
        if s2.shape != t2.shape or s2.shape[0] == 0:
            raise ValueError(f"kd_hidden_loss: shapes {tuple(s.shape)} and {tuple(t.shape)} do not pair")
        d = _KDHiddenFn.apply(s2, t2)
        total = d if total is None else total + d
    return total


class KDLoss(nn.Module):
    """The reference's ``KDTrainer.compute_loss`` as a module; defaults of ``hparams/model_args.py:81-100``."""

    def __init__(self, kd_alpha: float = 0.8, kd_beta: float = 0.0, kd_loss_scale: float = 1.0, kd_gamma: float = 0.0,
                 ignore_index: int = -100):
        super().__init__()
        if kd_gamma > 0:
            raise NotImplementedError(
                "kd_gamma > 0 (the attention-weight term) needs materialised [B, H, S, S] attention weights; "
                "this project's attention kernels never form them")
        self.kd_alpha, self.kd_beta, self.kd_loss_scale, self.kd_gamma = kd_alpha, kd_beta, kd_loss_scale, kd_gamma
        self.ignore_index = ignore_index

    def forward(self, student_logits, teacher_logits, labels, student_hidden_states=None, teacher_hidden_states=None,
                n_layers=None):
        loss, _, _ = kd_token_loss(student_logits, teacher_logits, labels, kd_alpha=self.kd_alpha,
                                   kd_loss_scale=self.kd_loss_scale, ignore_index=self.ignore_index)
        if self.kd_beta > 0:
            if student_hidden_states is None or teacher_hidden_states is None:
                raise ValueError("KDLoss: kd_beta > 0 needs the student's and the teacher's hidden states")
            n = len(student_hidden_states) - 1 if n_layers is None else n_layers
            # entries 0 .. n_layers - 1: the embedding output and all but the last layer's output (the reference's loop)
            loss = loss + self.kd_beta * kd_hidden_loss(student_hidden_states[:n], teacher_hidden_states[:n])
        return loss
