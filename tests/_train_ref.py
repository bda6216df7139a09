"""Element-wise checking of the train-mode layer -- helper of tests/test_train_ref_cpu.py and tests/test_gpu_train_elementwise.py.

The truth is oracle/train_ref.py (the torch-ops restatement pinned by tests/golden/train_bitlinear.npz) evaluated in float64 on
the CPU, on inputs that are exactly representable in the tensor dtype.  The BARS come from the same restatement evaluated on the
CPU in the tensor dtype: ``margin x`` its own distance to the float64 truth, per tensor and per metric.  Nothing here is measured
on the kernels.

Two metrics per tensor:

    peak(a, b) = max |a - b| / rms(b)      one wrong element is O(1); round-off is a few 1e-6 (fp32) / a few 1e-3 (fp16)
    l2(a, b)   = ||a - b|| / ||b||         the whole-tensor bar of tests/test_gpu_train.py

MARGIN = 4 covers another summation order of the same kind of arithmetic: the CPU BLAS and the MFMA blocks (4, 16 or 32 deep) both
accumulate in fp32, so the kernels' results are another realisation of the same rounding noise; tests/test_train_ref_cpu.py shows
that a reordered evaluation of the restatement itself stays inside it.  There is no absolute floor: a tensor the restatement gets
exactly (the bias gradient of a one-token batch) has to be exact.  The one exception is a tensor that is zero in exact arithmetic
(GRAPHS: the gradients under y.sum()), which has no scale of its own.
"""
import functools

import torch
import torch.nn.functional as F

MARGIN = 4.0
DTYPES = {"float32": torch.float32, "float16": torch.float16}
TENSORS = ("y", "gx", "weight", "weight_scale", "input_factor", "bias")       # the parameter names stand for their gradients

# (T, K, N) -- what each shape reaches in csrc/ob_train.h
SHAPES = [
    (1, 33, 65),        # one token; every reduction one past a 32-deep step (K forward, N in ga) or a single term (T in gW)
    (31, 40, 63),       # T below OB_TC_SLICES: slices without rows; N one short of a 64 tile
    (33, 67, 257),      # T one over the slice count (per = 2: slices with t1 < t0); odd K: rows that are not 16-byte aligned in fp32
                        # either; N one past four 64 tiles / two 128 tiles
    (129, 130, 131),    # ragged in every role, one past a 128 tile
    (65, 264, 136),     # multiples of 8: the 16-byte fetches with partial tiles
    (257, 96, 72),      # T as the reduction of gW, one past a step, through the transposed loaders of both operands
]
# id -> make_case arguments (without the dtype)
CASES = {}
for _i, (_T, _K, _N) in enumerate(SHAPES):
    for _bias in (True, False):
        CASES[f"{_T}x{_K}x{_N}-{'bias' if _bias else 'nobias'}"] = dict(T=_T, K=_K, N=_N, bias=_bias, seed=100 + _i)
for _i, (_T, _K, _N) in enumerate([(33, 67, 257), (129, 130, 131)]):
    CASES[f"{_T}x{_K}x{_N}-zero_row"] = dict(T=_T, K=_K, N=_N, bias=True, seed=200 + _i, zero_row=True)
    CASES[f"{_T}x{_K}x{_N}-saturate"] = dict(T=_T, K=_K, N=_N, bias=True, seed=300 + _i, saturate=True)
CASE_IDS = list(CASES)
SATURATED = 4.0         # |w| >= 4: 1.001 - tanh(w)^2 <= 2.4e-3, a cancellation


def make_case(T, K, N, dtype, bias, seed, *, zero_row=False, saturate=False):
    """parameters, x and coef of one case as float64 tensors whose values are exactly representable in `dtype`"""
    g = torch.Generator().manual_seed(seed)
    q = lambda t: t.to(dtype).double()
    weight = 0.3 * torch.randn(N, K, generator=g)
    weight[0, :3] = 0.0                                     # exact zeros: sign(0) = 0, STE factor 1.001
    if saturate:
        weight[::3, ::5] *= 20.0
    sgn = torch.where(torch.rand(N, generator=g) < 0.2, -1.0, 1.0)
    case = {"weight": q(weight),
            "weight_scale": q(0.1 * (0.5 + torch.rand(N, generator=g)) * sgn),
            "input_factor": q(0.1 * (0.5 + torch.rand(K, generator=g)))}
    if bias:
        case["bias"] = q(0.1 * torch.randn(N, generator=g))
    x = torch.randn(T, K, generator=g)
    if zero_row:
        assert T >= 2
        x[T // 2] = 0.0                                     # variance 0: rstd = 1 / sqrt(eps)
    case["x"], case["coef"] = q(x), q(torch.randn(T, N, generator=g))
    case["dims"] = (T, K, N)
    case["key"] = (T, K, N, str(dtype), bias, seed, zero_row, saturate)
    return case


@functools.lru_cache(maxsize=None)
def get_case(case_id, dtype_name):
    return make_case(dtype=DTYPES[dtype_name], **CASES[case_id])


# ---- the graphs: what is done with the layer.  fn(layer, x, coef) -> (y, loss) ------------------------------------------------
def _g_default(m, x, coef):
    y = m(x)
    return y, (y * coef).sum()


def _g_sum(m, x, coef):                                    # the gradient of a plain sum is a stride-0 expansion of one scalar
    y = m(x)
    return y, y.sum()


def _g_transposed(m, x, coef):                             # the layer is handed a non-contiguous [T, K] view of [K, T] storage
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous() or min(xt.shape) == 1
    y = m(xt)
    return y, (y * coef).sum()


def _g_row_broadcast(m, x, coef):                          # gy = one row expanded over the tokens: strides (0, 1)
    y = m(x)
    return y, (y.sum(0) * coef[0]).sum()


def _g_twice(m, x, coef):                                  # two uses of the layer in one graph: every gradient accumulates
    y = m(x)
    y2 = m(x.flip(0) * 0.5)
    return y, (y * coef).sum() + (y2 * coef.flip(1)).sum()


# name -> (fn, x requires grad, frozen parameters, tensors that are zero in exact arithmetic)
# The sum of a LayerNorm's outputs does not depend on its input, so under y.sum() every gradient except the bias's is zero in
# exact arithmetic and round-off in any other: those tensors have no scale of their own and are held to an ABSOLUTE bar, margin x
# the largest magnitude the restatement leaves there in the tensor dtype (metric "abs").
_LN_NULL = ("gx", "weight", "weight_scale", "input_factor")
GRAPHS = {
    "default": (_g_default, True, (), ()),
    "sum": (_g_sum, True, (), _LN_NULL),
    "row_broadcast": (_g_row_broadcast, True, (), ()),
    "transposed_x": (_g_transposed, True, (), ()),
    "x_no_grad": (_g_default, False, (), ()),
    "frozen_vectors": (_g_default, True, ("weight_scale", "input_factor"), ()),
    "twice": (_g_twice, True, (), ()),
}


def run_layer(cls, case, dtype, device="cpu", graph="default", split_k=False):
    """forward and backward of `cls` (oracle.train_ref.BitLinear or onebit_amd.train.BitLinear) on `case` in `dtype`:
    ({name: tensor as float64 on the CPU, or None where the graph asks for no gradient}, the layer, the input leaf).
    split_k (the restatement only): the same arithmetic with K summed in another order, two halves added afterwards."""
    fn, x_grad, frozen, _ = GRAPHS[graph]
    T, K, N = case["dims"]
    m = cls(K, N, bias="bias" in case, dtype=dtype).to(device)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(case[n].to(dtype))
            p.requires_grad_(n not in frozen)
    if split_k:
        def fwd(x, m=m):
            a, s, k2 = x * m.input_factor.view(1, K), m.sign(m.weight), K // 2
            out = F.linear(a[:, :k2], s[:, :k2]) + F.linear(a[:, k2:], s[:, k2:])
            out = m.layernorm(out * m.weight_scale.view(1, N))
            return out if m.bias is None else out + m.bias
        layer = fwd
    else:
        layer = m
    x = case["x"].to(dtype).to(device).clone().requires_grad_(x_grad)
    y, loss = fn(layer, x, case["coef"].to(dtype).to(device))
    loss.backward()
    out = {"y": y.detach(), "gx": x.grad}
    for n in ("weight", "weight_scale", "input_factor", "bias"):
        p = getattr(m, n)
        out[n] = None if p is None else p.grad
    assert all((out[n] is None) == (n in frozen) for n in ("weight", "weight_scale", "input_factor"))
    assert (out["gx"] is None) == (not x_grad)
    return {n: None if v is None else v.detach().double().cpu() for n, v in out.items()}, m, x


_REF = {}


def reference(case, dtype, graph="default", split_k=False):
    """oracle.train_ref.BitLinear on the CPU in `dtype`: y, gx and the parameter gradients as float64 (loss (y * coef).sum()).
    torch.float64 is the truth; the tensor dtype gives the restatement's own rounding.  Evaluated once per case and kept: do not
    modify what it returns."""
    from oracle.train_ref import BitLinear as RefBitLinear
    key = (case["key"], str(dtype), graph, split_k)
    if key not in _REF:
        _REF[key] = run_layer(RefBitLinear, case, dtype, "cpu", graph, split_k)[0]
    return _REF[key]


def rms(b):
    return float(b.double().pow(2).mean().sqrt())


def peak(a, b):
    """max |a - b| / rms(b)"""
    return float((a.double() - b.double()).abs().max()) / max(rms(b), 1e-300)


def l2(a, b):
    """||a - b|| / ||b||"""
    return float((a.double() - b.double()).norm()) / max(float(b.double().norm()), 1e-300)


def peak_on(a, b, mask):
    """peak with both the maximum and the rms restricted to `mask`"""
    return peak(a.double()[mask], b.double()[mask])


def saturated_mask(case):
    return case["weight"].abs() >= SATURATED


def metrics(got, truth, case=None, graph="default"):
    """{(tensor, metric): value} of `got` against `truth` (both from run_layer / reference); tensors without a gradient are left
    out.  With a saturated case, ("weight", "peak_sat") is peak_on over its saturated positions."""
    out = {}
    for n in TENSORS:
        if truth.get(n) is None:
            assert got.get(n) is None, n
            continue
        assert got[n] is not None and got[n].shape == truth[n].shape, n
        if n in GRAPHS[graph][3]:
            assert float(truth[n].abs().max()) <= 1e-9 * max(1.0, rms(truth["y"])), (n, "not zero in float64")
            out[(n, "abs")] = float(got[n].abs().max())
            continue
        assert float(truth[n].abs().max()) > 0, (n, "identically zero: needs an absolute bar, no case has one")
        out[(n, "peak")], out[(n, "l2")] = peak(got[n], truth[n]), l2(got[n], truth[n])
    if case is not None and case["key"][-1]:
        out[("weight", "peak_sat")] = peak_on(got["weight"], truth["weight"], saturated_mask(case))
    return out


def bars(case, dtype, margin=MARGIN, graph="default"):
    """{(tensor, metric): margin x the metric of reference(case, dtype) against reference(case, float64)}"""
    own = metrics(reference(case, dtype, graph), reference(case, torch.float64, graph), case, graph)
    return {k: margin * v for k, v in own.items()}
