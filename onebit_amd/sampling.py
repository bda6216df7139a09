"""Sampled decoding: the per-request parameters, their device rows and the standalone sampler.

``SamplingParams`` is HuggingFace ``generate(do_sample=True, temperature=..., top_k=..., top_p=...)``'s warper chain
(``TemperatureLogitsWarper`` -> ``TopKLogitsWarper`` -> ``TopPLogitsWarper``, in ``_get_logits_warper`` order) followed by a
draw.  The draw is a Gumbel-max over Philox4x32-10 noise keyed by (seed, stream, n, token): the token is a pure function of
the logits row, the parameters and the index ``n`` of the generated token in its sequence (include/onebit.h states the
contract).  It samples from the same warped softmax as HF, but not with torch's RNG stream.
"""
from __future__ import annotations

import ctypes
import math
import numbers
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import torch

from . import _lib


class SampleParamsStruct(ctypes.Structure):      # onebit_sample_params_t (ABI 10), 32 bytes
    _fields_ = [("do_sample", ctypes.c_int32), ("temperature", ctypes.c_float), ("top_k", ctypes.c_int32), ("top_p", ctypes.c_float),
                ("seed_lo", ctypes.c_uint32), ("seed_hi", ctypes.c_uint32), ("stream", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


@dataclass
class SamplingParams:
    """One request's sampling.  Defaults are ``GenerationConfig``'s (temperature 1, top_k 50, top_p 1).  ``seed``: a 64-bit key of
    the Philox noise; None draws one from torch's default CPU generator (``torch.manual_seed`` makes runs repeatable, as HF's
    ``set_seed`` does).  ``stream``: a 32-bit counter word; rows that share a seed differ by their stream."""
    temperature: float = 1.0
    top_k: int = 50
    top_p: float = 1.0
    seed: Optional[int] = None
    stream: int = 0

    def __post_init__(self):
        # as the HF warpers validate (generation/logits_process.py: Temperature / TopK / TopP LogitsWarper)
        # numbers.Real / Integral: numpy scalars are taken as HF's warpers take them
        t = self.temperature
        if isinstance(t, bool) or not isinstance(t, numbers.Real) or not (t > 0) or not math.isfinite(t):
            raise ValueError(f"`temperature` has to be a strictly positive float, but is {t}")
        if isinstance(self.top_k, bool) or not isinstance(self.top_k, numbers.Integral) or self.top_k < 0:
            raise ValueError(f"`top_k` has to be a non-negative integer, but is {self.top_k}")
        p = self.top_p
        if isinstance(p, bool) or not isinstance(p, numbers.Real) or not (0.0 <= p <= 1.0):
            raise ValueError(f"`top_p` has to be a float >= 0 and <= 1, but is {p}")
        self.temperature, self.top_k, self.top_p = float(t), int(self.top_k), float(p)
        if self.seed is None:
            self.seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
        if isinstance(self.seed, bool) or not isinstance(self.seed, numbers.Integral) or not 0 <= int(self.seed) < 2 ** 64:
            raise ValueError(f"`seed` has to be an integer in [0, 2**64), but is {self.seed}")
        if isinstance(self.stream, bool) or not isinstance(self.stream, numbers.Integral) or not 0 <= int(self.stream) < 2 ** 32:
            raise ValueError(f"`stream` has to be an integer in [0, 2**32), but is {self.stream}")
        self.seed, self.stream = int(self.seed), int(self.stream)

    def with_stream(self, stream: int) -> "SamplingParams":
        return SamplingParams(self.temperature, self.top_k, self.top_p, self.seed, int(stream))

    def struct(self) -> SampleParamsStruct:
        return SampleParamsStruct(1, float(self.temperature), int(self.top_k), float(self.top_p),
                                  self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF, self.stream, 0)


GREEDY = SampleParamsStruct(0, 1.0, 0, 1.0, 0, 0, 0, 0)


def pack_host(params: Sequence[Optional[SamplingParams]]) -> torch.Tensor:
    """The rows as a CPU uint8 tensor [len, 32] (None: a greedy row)."""
    arr = (SampleParamsStruct * max(len(params), 1))()
    for i, p in enumerate(params):
        arr[i] = p.struct() if p is not None else GREEDY
    raw = bytes(arr)[:32 * len(params)]
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(len(params), 32) if params else torch.zeros(0, 32, dtype=torch.uint8)


def pack(params: Sequence[Optional[SamplingParams]], device) -> torch.Tensor:
    """Device rows of onebit_sample_params_t (uint8 [len, 32]) for ``params``; None is a greedy row."""
    return pack_host(params).to(device)


def sample_logits(logits: torch.Tensor, params: Union[SamplingParams, Sequence[Optional[SamplingParams]], torch.Tensor],
                  positions) -> torch.Tensor:
    """The sampler over fp16 logits [R, V] (V <= 65536): int32 [R] tokens, row r drawn with params[r] at n = positions[r].
    ``params``: one SamplingParams for every row, a list (None = greedy row) or packed device rows (``pack``)."""
    if logits.dim() != 2 or logits.dtype != torch.float16 or not logits.is_cuda:
        raise ValueError("sample_logits: logits must be a CUDA fp16 tensor [R, V]")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    R, V = logits.shape
    dev = logits.device
    if isinstance(params, SamplingParams):
        params = [params] * R
    if not isinstance(params, torch.Tensor):
        if len(params) != R:
            raise ValueError("sample_logits: one params entry per row")
        params = pack(params, dev)
    if params.dtype != torch.uint8 or params.shape != (R, 32) or not params.is_contiguous() or params.device != dev:
        raise ValueError("sample_logits: packed params must be contiguous uint8 [R, 32] on the logits' device")
    pos = torch.as_tensor(positions, dtype=torch.int32).reshape(-1).to(dev)
    if pos.numel() != R:
        raise ValueError("sample_logits: one position per row")
    out = torch.empty(R, dtype=torch.int32, device=dev)
    if R == 0:
        return out
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.onebit_sample_rows(logits.data_ptr(), logits.stride(0), V, R, params.data_ptr(), pos.data_ptr(), out.data_ptr(),
                                    torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "onebit_sample_rows")
    return out
