"""The train-mode layer (onebit_amd/train.py -> onebit_train_forward / onebit_train_backward, csrc/ob_train.h) element by element
against oracle/train_ref.py evaluated in float64 on the CPU, at the smallest shapes that reach each branch of the kernels
(tests/_train_ref.py: SHAPES), in fp32 and fp16.

Every bar is ``margin x`` the distance of the SAME restatement, evaluated on the CPU in the tensor dtype, to that truth -- per
tensor, for max |a - b| / rms(b) and for the relative L2 (tests/_train_ref.py says why the margin is 4; tests/test_train_ref_cpu.py
shows what the two metrics catch).  No number here comes from the kernels.  The measured values are written next to their bars
(profiles/train_elementwise.txt, or that file under the directory OB_PROFILES_DIR names) when OB_WRITE_PROFILES=1."""
import os

import pytest
import torch

import _train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5                                       # nn.LayerNorm's default, what BitLinear hands the kernels

# (dtype, tensor) -> margin, where it is not R.MARGIN.  None is set.
MARGINS = {}


def _log(case_id, dtype_name, what, got, bar):
    if os.environ.get("OB_WRITE_PROFILES") != "1":
        return
    out_dir = os.environ.get("OB_PROFILES_DIR") or os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    route = "gemm64" if os.environ.get("OB_TRAIN_GEMM64") is not None else "default"
    with open(os.path.join(out_dir, "train_elementwise.txt"), "a") as f:
        for (n, metric), v in got.items():
            b = bar[(n, metric)]
            f.write(f"{case_id:<26s} {dtype_name:<8s} {route:<8s} {what:<15s} {n:<13s} {metric:<9s} measured {v:.3e}  bar {b:.3e}  "
                    f"ratio {v / b if b > 0 else (0.0 if v == 0 else float('inf')):.3f}\n")


def _bars(case, dtype_name, graph="default"):
    bar = R.bars(case, R.DTYPES[dtype_name], graph=graph)
    return {k: v * MARGINS.get((dtype_name, k[0]), R.MARGIN) / R.MARGIN for k, v in bar.items()}


_MODULE = {}


def _module_run(case_id, dtype_name):
    """train.BitLinear forward and backward on the case, once per (case, dtype) of this process"""
    from onebit_amd.train import BitLinear
    key = (case_id, dtype_name)
    if key not in _MODULE:
        _MODULE[key] = R.run_layer(BitLinear, R.get_case(case_id, dtype_name), R.DTYPES[dtype_name], DEV)[0]
    return _MODULE[key]


def _assert_within(case_id, dtype_name, what, got, truth, case, graph="default"):
    for n, v in got.items():
        assert v is None or bool(torch.isfinite(v).all()), (n, "not finite")
    bar = _bars(case, dtype_name, graph)
    m = R.metrics(got, truth, case, graph)
    assert m.keys() == bar.keys()
    _log(case_id, dtype_name, what, m, bar)
    for k in bar:
        print(case_id, dtype_name, what, k, "measured %.3e  bar %.3e" % (m[k], bar[k]))
    bad = {k: (m[k], bar[k]) for k in bar if not m[k] <= bar[k]}
    assert not bad, bad


# ---- a. element-wise parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", list(R.DTYPES))
@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_elementwise_parity(case_id, dtype_name):
    from onebit_amd.train import BitLinear
    case = R.get_case(case_id, dtype_name)
    got = _module_run(case_id, dtype_name)
    _assert_within(case_id, dtype_name, "module", got, R.reference(case, torch.float64), case)
    # deterministic: a second layer, forward and backward, gives the same bits
    again = R.run_layer(BitLinear, case, R.DTYPES[dtype_name], DEV)[0]
    for n, v in got.items():
        assert (v is None and again[n] is None) or torch.equal(v, again[n]), n


# ---- b. writes stay inside their buffers; the workspace is written before it is read ---------------------------------------------
GUARD = 4096
SENTINEL = 0xFF                                  # 0xFFFF / 0xFFFFFFFF: NaN in fp16 and fp32


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.parametrize("dtype_name", list(R.DTYPES))
@pytest.mark.parametrize("case_id", ["33x67x257-bias", "33x67x257-nobias", "31x40x63-bias", "31x40x63-nobias"])
def test_c_abi_writes_stay_inside_and_workspace_is_written_before_read(case_id, dtype_name):
    from onebit_amd import _lib
    from onebit_amd.bitnet import _dtype_code, _stream_ptr
    lib = _lib.load()
    dtype = R.DTYPES[dtype_name]
    case = R.get_case(case_id, dtype_name)
    T, K, N = case["dims"]
    sz, code = (4 if dtype == torch.float32 else 2), _dtype_code(dtype)
    has_bias = "bias" in case
    nws = lib.onebit_train_workspace_bytes(T, K, N, code)
    assert nws > 0
    # every output and the workspace carved out of one arena of sentinel bytes: outputs where torch's allocator would put them
    # (512-byte aligned), the workspace 16-byte aligned and no better, exactly as long as stated; >= 4 KiB of sentinel around each
    spec = [("y", T * N * sz), ("z", T * N * sz), ("stats", T * 2 * 4), ("gx", T * K * sz), ("gw", N * K * sz), ("gh", K * sz),
            ("gg", N * sz)] + ([("gbias", N * sz)] if has_bias else []) + [("ws", nws)]
    off, spans = GUARD, {}
    for name, nbytes in spec:
        off = (off + 511) // 512 * 512 + (16 if name == "ws" else 0)
        spans[name] = (off, nbytes)
        off += nbytes + GUARD
    total = off
    arena = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
    base = arena.data_ptr()
    assert base % 512 == 0 and (base + spans["ws"][0]) % 32 == 16
    ptr = {n: base + o for n, (o, _) in spans.items()}
    dev = torch.device(DEV)
    t = {n: case[n].to(dtype).to(DEV).contiguous() for n in ("x", "weight", "input_factor", "weight_scale", "coef")}
    b = case["bias"].to(dtype).to(DEV).contiguous() if has_bias else None
    with torch.cuda.device(dev):
        s = _stream_ptr(dev)
        rc = lib.onebit_train_forward(t["x"].data_ptr(), t["weight"].data_ptr(), t["input_factor"].data_ptr(), t["weight_scale"].data_ptr(),
                                      None if b is None else b.data_ptr(), ptr["y"], ptr["z"], ptr["stats"], T, K, N, code, EPS, s)
        _lib.check(rc, "onebit_train_forward")
        rc = lib.onebit_train_backward(t["coef"].data_ptr(), t["x"].data_ptr(), t["weight"].data_ptr(), t["input_factor"].data_ptr(),
                                       t["weight_scale"].data_ptr(), ptr["z"], ptr["stats"], ptr["gx"], ptr["gw"], ptr["gh"], ptr["gg"],
                                       ptr["gbias"] if has_bias else None, ptr["ws"], nws, T, K, N, code, s)
        _lib.check(rc, "onebit_train_backward")
    torch.cuda.synchronize()
    host = arena.cpu()
    # every guard byte is unchanged
    guard = torch.ones(total, dtype=torch.bool)
    for o, nbytes in spans.values():
        guard[o:o + nbytes] = False
    assert int(guard.sum()) >= GUARD * (len(spec) + 1)
    touched = torch.nonzero(guard & (host != SENTINEL)).flatten()
    assert touched.numel() == 0, ("bytes written outside the buffers", touched[:8].tolist(), spans)

    def carve(name, dt, shape):
        o, nbytes = spans[name]
        return host[o:o + nbytes].clone().view(dt).view(shape)
    out = {"y": carve("y", dtype, (T, N)), "z": carve("z", dtype, (T, N)), "stats": carve("stats", torch.float32, (T, 2)),
           "gx": carve("gx", dtype, (T, K)), "weight": carve("gw", dtype, (N, K)), "input_factor": carve("gh", dtype, (K,)),
           "weight_scale": carve("gg", dtype, (N,))}
    if has_bias:
        out["bias"] = carve("gbias", dtype, (N,))
    # every output element was written (the sentinel is NaN), with a finite value: nothing the backward pass read was sentinel
    for n, v in out.items():
        assert bool(torch.isfinite(v).all()), (n, "sentinel or non-finite elements", int((~torch.isfinite(v)).sum()))
    # ... and equals, bit for bit, what the module path gives for the same case
    ref = _module_run(case_id, dtype_name)
    for n in R.TENSORS:
        if ref[n] is None:
            assert n not in out
            continue
        assert torch.equal(_bits(out[n]), _bits(ref[n].to(dtype))), (n, "differs from the module path", int((out[n].double() != ref[n]).sum()))


# ---- c. autograd plumbing that changes what the kernels are handed --------------------------------------------------------------
PLUMBING_CASE = "33x67x257-bias"


@pytest.mark.parametrize("graph", [g for g in R.GRAPHS if g != "default"])
def test_autograd_plumbing_fp32(graph):
    from onebit_amd.train import BitLinear
    case = R.get_case(PLUMBING_CASE, "float32")
    got = R.run_layer(BitLinear, case, torch.float32, DEV, graph)[0]
    _assert_within(PLUMBING_CASE, "float32", graph, got, R.reference(case, torch.float64, graph), case, graph)
    if graph in ("transposed_x", "x_no_grad", "frozen_vectors"):      # the same kernels on the same numbers as the plain graph
        plain = _module_run(PLUMBING_CASE, "float32")
        for n, v in got.items():
            assert v is None or torch.equal(v, plain[n]), n


def test_non_default_stream_fp32():
    from onebit_amd.train import BitLinear
    case = R.get_case(PLUMBING_CASE, "float32")
    plain = _module_run(PLUMBING_CASE, "float32")
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        got = R.run_layer(BitLinear, case, torch.float32, DEV)[0]
    s.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(s)
    _assert_within(PLUMBING_CASE, "float32", "side_stream", got, R.reference(case, torch.float64), case)
    for n, v in got.items():
        assert v is None or torch.equal(v, plain[n]), n
