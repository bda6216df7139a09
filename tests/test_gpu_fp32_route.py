"""The fp32 route of the 1-bit linear layer (onebit_amd/csrc/ob_f32.h): GEMV for one token, tiled fp32-MFMA GEMM for more,
rows-in-registers LayerNorm -- against the C oracle (fp64 accumulation), against the generic kernel on the same inputs
(reached by copying the packed matrix into a buffer whose row pitch is K / 8 + 1), through the K-sharded entry points, on
the edges, under graph capture, and at model level against the reference's fp32 logits.

Layer bars: the project's own fp32 bars of test_goldens_forward, |u - u_ref| <= 2e-5 max|u_ref| and |y - y_ref| <= 2e-4, on
every element.  A single k-ordered fp32 chain -- one MFMA accumulator -- measures 3.8e-6 / 1.1e-5 of them at K = 11008 and
4.2e-6 / 1.1e-5 at K = 13824 against fp64, so the bars hold with a 5x margin for any summation order at least that good.

Model bars: a tenth of the fixture's own max|ref_f16 - ref_f32| -- an fp32 route must sit clearly on the fp32 side of that
gap; fp32 round-off is three orders of magnitude below fp16's.  Measured max|logits - ref_f32| (profiles/fp32_route.txt;
generic kernel of the parent commit / this route, MI355X):
    model_wide_c  prefill 12 tokens   gap 6.04e-3  bar 6.04e-4   parent 5.3e-6   here 8.3e-6
    model_wide_c  4 decode steps      gap 6.32e-3  bar 6.32e-4   parent 4.8e-6   here 7.0e-6
    model_wide_c  4096-token prompt   gap 6.01e-3  bar 6.01e-4   parent not run (45 M workgroups per projection)   here 4.5e-5
    model_tiny_a  prefill / decode    gap 1.48e-3 / 1.61e-3      parent 6.6e-7 / 4.8e-7   here 7.7e-7 / 7.2e-7
    model_tiny_b  prefill / decode    gap 1.17e-3 / 1.05e-3      parent 5.1e-7 / 4.2e-7   here 5.4e-7 / 4.2e-7
The parent's generic route is two orders of magnitude below a tenth of the gap on every part it can run, so no part takes the
"twice the parent" bar.
The parts are also held to the fp16 golden at the tests/_parity_log.py bar.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = 1
E_FLAG = -6
FLAG_SKIP_LN, FLAG_PRESCALED, FLAG_TILE_STATS = 1, 4, 8
U_BAR, Y_BAR = 2e-5, 2e-4
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    from onebit_amd import _lib
    _lib.load()                      # native library must be present: no fallback
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _inputs(seed, T, K, N, bias):
    rng = np.random.default_rng(seed)
    packed = rng.integers(0, 256, (N, max(K // 8, 0)), dtype=np.uint8).view(np.int8)
    x = rng.standard_normal((T, K)).astype(np.float32)
    h = (0.5 + rng.random(K)).astype(np.float32)
    g = (0.5 + rng.random(N)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32) if bias else None
    return packed, x, h, g, b


def _oracle(coracle, packed, x, h, g, b):
    """coracle.forward_f32 (fp64 accumulation) with the tokens spread over 16 threads (ctypes releases the GIL)."""
    T = x.shape[0]
    if T * x.shape[1] * packed.shape[0] < 1 << 28:
        return coracle.forward_f32(packed, x, h, g, b, return_pre_ln=True)
    parts = [p for p in np.array_split(np.arange(T), min(T, 16)) if len(p)]
    with ThreadPoolExecutor(16) as ex:
        res = list(ex.map(lambda p: coracle.forward_f32(packed, x[p[0]:p[-1] + 1], h, g, b, return_pre_ln=True), parts))
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def _odd_pitch(pt):
    """The same packed rows at pitch K / 8 + 1 bytes: onebit_linear_f32_route answers 0, the generic kernel runs."""
    N, KB = pt.shape
    buf = torch.zeros(N, KB + 1, dtype=torch.int8, device=pt.device)
    buf[:, :KB] = pt
    return buf


def _forward(lib, w, ldw, x, h, g, b, N, flags=0, want_u=False, rc_only=False):
    from onebit_amd.bitnet import _stream_ptr
    T, K = x.shape
    y = torch.full((T, N), float("nan"), dtype=torch.float32, device=x.device)
    u = torch.full((T, N), float("nan"), dtype=torch.float32, device=x.device) if want_u else None
    rc = lib.onebit_linear_forward(w.data_ptr(), ldw, x.data_ptr(), h.data_ptr(), g.data_ptr(), None if b is None else b.data_ptr(),
                                   y.data_ptr(), None if u is None else u.data_ptr(), None, 0, T, K, N, F32, EPS, flags,
                                   _stream_ptr(x.device))
    if rc_only:
        return rc
    from onebit_amd import _lib
    _lib.check(rc, "onebit_linear_forward")
    return (y, u) if want_u else y


def _check(u, y, u_ref, y_ref, tag):
    """every element, no exclusions; figures printed before they are asserted"""
    eu = float(np.abs(u - u_ref).max()) / (float(np.abs(u_ref).max()) + 1e-30)
    ey = float(np.abs(y - y_ref).max())
    print(f"fp32 route {tag}: max|u - u_ref| / max|u_ref| = {eu:.3e} (bar {U_BAR:.0e})   max|y - y_ref| = {ey:.3e} (bar {Y_BAR:.0e})")
    assert np.isfinite(u).all() and np.isfinite(y).all(), tag
    assert eu <= U_BAR, (tag, "pre-LayerNorm u", eu)
    assert ey <= Y_BAR, (tag, "y", ey)


TS = [1, 2, 12, 17, 64, 129, 2048]
KNS = [(4096, 11008), (11008, 4096), (5120, 13824), (256, 130), (352, 48)]
# T = 2048 keeps one full-width shape (the 128 x 64 tile over several rounds of the chip) and the two small ones: the oracle is a
# scalar fp64 loop (T K N steps; 92 G for [2048, 4096] -> 11008, spread over 16 threads)
CASES = [(T, K, N, (i + j) % 2 == 1) for i, T in enumerate(TS) for j, (K, N) in enumerate(KNS)
         if not (T == 2048 and (K, N) in ((11008, 4096), (5120, 13824)))]
assert {c[0] for c in CASES} == set(TS) and {(c[1], c[2]) for c in CASES} == set(KNS)
assert any(c[3] for c in CASES) and not all(c[3] for c in CASES)


@pytest.mark.parametrize("T,K,N,bias", CASES)
def test_layer_vs_oracle(dev, coracle, T, K, N, bias):
    from onebit_amd import _lib
    lib = _lib.load()
    packed, x, h, g, b = _inputs(1000 * T + K + N, T, K, N, bias)
    y_ref, u_ref = _oracle(coracle, packed, x, h, g, b)
    pt, xt, ht, gt = (_t(a, dev) for a in (packed, x, h, g))
    bt = None if b is None else _t(b, dev)
    route = lib.onebit_linear_f32_route(T, K, N, K // 8)
    assert route == (1 if T == 1 and K % 128 == 0 else 2), route
    y, u = _forward(lib, pt, K // 8, xt, ht, gt, bt, N, want_u=True)               # y and u_or_null together
    _check(u.cpu().numpy(), y.cpu().numpy(), u_ref, y_ref, f"T={T} {K}->{N} bias={int(bias)} route {route}")
    y1 = _forward(lib, pt, K // 8, xt, ht, gt, bt, N)                              # y alone (u staged in y)
    assert torch.equal(y1, y)
    us = _forward(lib, pt, K // 8, xt, ht, gt, bt, N, flags=FLAG_SKIP_LN)          # pre-LayerNorm u in y
    assert torch.equal(us, u)
    ys, uu = _forward(lib, pt, K // 8, xt, ht, gt, bt, N, flags=FLAG_SKIP_LN, want_u=True)
    assert torch.equal(ys, u) and torch.equal(uu, u)
    assert torch.equal(_forward(lib, pt, K // 8, xt, ht, gt, bt, N), y)            # determinism: identical bytes


@pytest.mark.parametrize("T,K,N,bias", [(1, 4096, 11008, False), (2, 5120, 13824, True), (12, 11008, 4096, False), (17, 256, 130, True),
                                        (64, 352, 48, False), (129, 256, 130, False), (300, 4096, 1024, True)])
def test_same_inputs_both_routes(dev, coracle, T, K, N, bias):
    from onebit_amd import _lib
    lib = _lib.load()
    packed, x, h, g, b = _inputs(7 + T + K + N, T, K, N, bias)
    y_ref, u_ref = _oracle(coracle, packed, x, h, g, b)
    pt, xt, ht, gt = (_t(a, dev) for a in (packed, x, h, g))
    bt = None if b is None else _t(b, dev)
    podd = _odd_pitch(pt)
    assert lib.onebit_linear_f32_route(T, K, N, K // 8) in (1, 2)
    assert lib.onebit_linear_f32_route(T, K, N, podd.stride(0)) == 0 and podd.stride(0) == K // 8 + 1
    y, u = _forward(lib, pt, K // 8, xt, ht, gt, bt, N, want_u=True)
    yg, ug = _forward(lib, podd, podd.stride(0), xt, ht, gt, bt, N, want_u=True)
    y, u, yg, ug = (a.cpu().numpy() for a in (y, u, yg, ug))
    _check(u, y, u_ref, y_ref, f"T={T} {K}->{N} new route")
    _check(ug, yg, u_ref, y_ref, f"T={T} {K}->{N} generic kernel")
    d = float(np.abs(u - ug).max()) / float(np.abs(u_ref).max())
    print(f"fp32 route T={T} {K}->{N}: max|u_new - u_generic| / max|u_ref| = {d:.3e} (bar {2 * U_BAR:.0e})")
    assert d <= 2 * U_BAR


@pytest.mark.parametrize("T", [1, 12, 200])
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("ws", [False, True])
def test_k_sharded_partials_fp32(dev, T, S, ws):
    """onebit_matmul_partial(_ws) in fp32 over K slices of a wider x (ldx = 4096 > K) and of the packed matrix, summed and passed
    through onebit_scale_layernorm == the full forward, within the layer bars."""
    from onebit_amd import _lib
    from onebit_amd.bitnet import _stream_ptr
    lib = _lib.load()
    K, N = 4096, 1000
    packed, x, h, g, b = _inputs(31 + T + S, T, K, N, True)
    pt, xt, ht, gt, bt = (_t(a, dev) for a in (packed, x, h, g, b))
    y_full, u_full = _forward(lib, pt, K // 8, xt, ht, gt, bt, N, want_u=True)
    Ks = K // S
    assert lib.onebit_linear_f32_route(T, Ks, N, K // 8) == (1 if T == 1 else 2)
    zsum = torch.zeros(T, N, dtype=torch.float32, device=dev)
    wsb = torch.empty(4096, dtype=torch.uint8, device=dev)                       # a small workspace is accepted, as is none
    for s in range(S):
        zp = torch.full((T, N), float("nan"), dtype=torch.float32, device=dev)
        args = (pt.data_ptr() + s * Ks // 8, K // 8, xt.data_ptr() + 4 * s * Ks, K, ht.data_ptr() + 4 * s * Ks, zp.data_ptr())
        if ws:
            rc = lib.onebit_matmul_partial_ws(*args, wsb.data_ptr(), wsb.numel(), T, Ks, N, F32, _stream_ptr(dev))
        else:
            rc = lib.onebit_matmul_partial(*args, T, Ks, N, F32, _stream_ptr(dev))
        _lib.check(rc, "matmul_partial")
        zsum += zp
    y = torch.empty(T, N, dtype=torch.float32, device=dev)
    u = torch.empty(T, N, dtype=torch.float32, device=dev)
    _lib.check(lib.onebit_scale_layernorm(zsum.data_ptr(), gt.data_ptr(), bt.data_ptr(), y.data_ptr(), u.data_ptr(), T, N, F32, EPS, 0,
                                          _stream_ptr(dev)), "scale_layernorm")
    _check(u.cpu().numpy(), y.cpu().numpy(), u_full.cpu().numpy(), y_full.cpu().numpy(), f"K-sharded T={T} S={S} ws={int(ws)}")


@pytest.mark.parametrize("T,K,N", [(5, 256, 130), (3, 4096, 17), (1, 4096, 17), (40, 1024, 1), (1, 128, 1), (33, 96, 21)])
def test_ragged_rows(dev, coracle, T, K, N):
    from onebit_amd import _lib
    lib = _lib.load()
    packed, x, h, g, b = _inputs(5 + T + K + N, T, K, N, N > 1)
    y_ref, u_ref = coracle.forward_f32(packed, x, h, g, b, return_pre_ln=True)
    pt, xt, ht, gt = (_t(a, dev) for a in (packed, x, h, g))
    bt = None if b is None else _t(b, dev)
    assert lib.onebit_linear_f32_route(T, K, N, K // 8) in (1, 2)
    y, u = _forward(lib, pt, K // 8, xt, ht, gt, bt, N, want_u=True)
    if N == 1:                                                   # LayerNorm of one element is 0 whatever u is
        assert np.abs(u.cpu().numpy() - u_ref).max() <= U_BAR * np.abs(u_ref).max() and float(y.abs().max()) == 0.0
    else:
        _check(u.cpu().numpy(), y.cpu().numpy(), u_ref, y_ref, f"ragged T={T} {K}->{N}")


def test_empty_calls_flags_and_promotion(dev):
    from onebit_amd import BitLinearInf, _lib
    lib = _lib.load()
    K, N = 4096, 512
    packed, x, h, g, b = _inputs(3, 4, K, N, True)
    pt, xt, ht, gt, bt = (_t(a, dev) for a in (packed, x, h, g, b))
    # T = 0: nothing to do
    assert _forward(lib, pt, K // 8, xt[:0], ht, gt, bt, N, rc_only=True) == 0
    # K = 0: u = 0, y = bias (as on the generic route)
    x0 = torch.empty(4, 0, dtype=torch.float32, device=dev)
    y0, u0 = _forward(lib, pt, 0, x0, ht, gt, bt, N, want_u=True)
    assert float(u0.abs().max()) == 0.0 and torch.equal(y0, bt.expand(4, N))
    # the fp16-only flags stay refused
    assert _forward(lib, pt, K // 8, xt, ht, gt, bt, N, flags=FLAG_PRESCALED, rc_only=True) == E_FLAG
    assert _forward(lib, pt, K // 8, xt, ht, gt, bt, N, flags=FLAG_SKIP_LN | FLAG_TILE_STATS, want_u=True, rc_only=True) == E_FLAG
    # fp16 input with fp32 parameters promotes to fp32, as in the reference
    m = BitLinearInf(K, N, bias=True, dtype=torch.float32).to(dev)
    m.weight.data, m.input_factor.data, m.weight_scale.data, m.bias.data = pt, ht, gt, bt
    for xs in (xt, xt[:1]):
        y16 = m(xs.half())
        assert y16.dtype == torch.float32 and torch.equal(y16, m(xs.half().float()))
        assert torch.equal(m(xs), _forward(lib, pt, K // 8, xs.contiguous(), ht, gt, bt, N))     # the module takes the same route


@pytest.mark.parametrize("T", [1, 20, 150])
def test_nan_inf_positions_match_generic_route(dev, T):
    from onebit_amd import _lib
    lib = _lib.load()
    K, N = 1024, 200
    packed, x, h, g, b = _inputs(11 + T, T + 3, K, N, False)
    x[0, 5] = np.nan
    x[1, 700] = np.inf
    x[2, 33] = -np.inf
    x[2, 900] = np.inf                                           # +inf and -inf in one token: NaN
    pt, ht, gt = (_t(a, dev) for a in (packed, h, g))
    podd = _odd_pitch(pt)
    for xs in ([x[0:1], x[1:2], x[2:3]] if T == 1 else [x]):     # (T = 1: each special token alone)
        xt = _t(xs, dev)
        Tn = xt.shape[0]
        assert lib.onebit_linear_f32_route(Tn, K, N, K // 8) in (1, 2) and lib.onebit_linear_f32_route(Tn, K, N, K // 8 + 1) == 0
        y, u = _forward(lib, pt, K // 8, xt, ht, gt, None, N, want_u=True)
        yg, ug = _forward(lib, podd, K // 8 + 1, xt, ht, gt, None, N, want_u=True)
        for a, c in ((u, ug), (y, yg)):
            assert torch.equal(torch.isnan(a), torch.isnan(c))
            assert torch.equal(torch.isposinf(a), torch.isposinf(c)) and torch.equal(torch.isneginf(a), torch.isneginf(c))
        assert torch.isnan(u).any() or torch.isinf(u).any()
        if Tn > 3:
            assert torch.isfinite(u[3:]).all() and torch.isfinite(y[3:]).all()   # the other tokens are untouched


def test_graph_capture_and_replay(dev):
    """One tiled call and one GEMV call captured with torch.cuda.graph, each replayed twice: identical bytes."""
    from onebit_amd import _lib
    lib = _lib.load()
    K, N = 4096, 1024
    for T in (48, 1):
        packed, x, h, g, b = _inputs(17 + T, T, K, N, True)
        pt, xt, ht, gt, bt = (_t(a, dev) for a in (packed, x, h, g, b))
        assert lib.onebit_linear_f32_route(T, K, N, K // 8) == (1 if T == 1 else 2)
        eager = _forward(lib, pt, K // 8, xt, ht, gt, bt, N)      # (also the warm-up: no first-call set-up inside the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yc = _forward(lib, pt, K // 8, xt, ht, gt, bt, N)
        for _ in range(2):
            yc.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(yc, eager)


# ------------------------------------------------------------------------------------------------------------- model level --

def _model_bar(z, name):
    return 0.1 * float(np.abs(z[name + "_f16"] - z[name + "_f32"]).max())


def _model_check(fixture, z, name, got, sl=None):
    from _parity_log import check, loose_tol
    r16, r32 = z[name + "_f16"], z[name + "_f32"]
    loose = loose_tol(r16, r32)
    bar = _model_bar(z, name)
    if sl is not None:
        r16, r32 = r16[sl], r32[sl]
    got = got.reshape(r32.shape).astype(np.float32)
    e32 = float(np.abs(got - r32).max())
    print(f"fp32 module path {fixture} {name}: max|logits - ref_f32| = {e32:.3e} (bar {bar:.3e}; reference's fp16-fp32 gap {10 * bar:.3e}, "
          f"logit scale {float(np.abs(z[name + '_f32']).max()):.3f})")
    assert e32 <= bar, (fixture, name, e32, bar)
    check(fixture, name, "fp32 module path", got, r16, r32, loose=loose)     # and the fp16 golden at the existing bar


def _all_projections_on_new_route(model, T):
    from onebit_amd import BitLinearInf, _lib
    lib = _lib.load()
    routes = {lib.onebit_linear_f32_route(T, m.in_features, m.out_features, m.weight.stride(0)) for m in model.modules() if isinstance(m, BitLinearInf)}
    return routes


def test_model_wide_fp32_vs_reference(dev, golden_dir):
    """OneBitLlamaForCausalLM(cfg, torch.float32) at 7B widths (2 layers) built as the reference's fp32 model was
    (tests/golden/gen_goldens_model_wide.py:75-89): 12-token prefill, 4 decode steps fed the reference's fp32 greedy tokens, and the
    4096-token prompt at its recorded positions."""
    from onebit_amd.llama import OneBitLlamaConfig, OneBitLlamaForCausalLM, synthetic_state_dict
    z = np.load(os.path.join(golden_dir, "model_wide_c.npz"))
    kw = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg_")}
    cfg = OneBitLlamaConfig(**kw)
    sd16 = synthetic_state_dict(cfg, seed=int(z["seed"]), dtype=torch.float16, device="cpu")
    model = OneBitLlamaForCausalLM(cfg, torch.float32)
    model.load_state_dict({k: (v if v.dtype == torch.int8 else v.float()) for k, v in sd16.items()})
    model = model.to(dev).eval()
    assert _all_projections_on_new_route(model, 12) == {2} and _all_projections_on_new_route(model, 1) == {1}
    ids = torch.from_numpy(z["input_ids"]).to(dev)
    with torch.no_grad():
        cache = model.new_cache(1, 32)
        lg = model(ids, cache)
        assert lg.dtype == torch.float32
        _model_check("model_wide_c", z, "prefill_logits", lg.cpu().numpy())
        toks = torch.from_numpy(z["greedy_f32"]).to(dev)
        assert int(lg[0, -1].argmax()) == int(toks[0, 0])
        dec = np.concatenate([model(toks[:, i:i + 1], cache).cpu().numpy() for i in range(4)], axis=1)
        _model_check("model_wide_c", z, "decode_logits", dec)
        lids = torch.from_numpy(z["long_ids"]).to(dev)
        T = lids.shape[1]
        assert _all_projections_on_new_route(model, T) == {2}
        lg = model(lids, model.new_cache(1, T))[0, torch.from_numpy(z["long_pos"]).to(dev)]
        _model_check("model_wide_c", z, "long_logits", lg.cpu().numpy())


@pytest.mark.parametrize("name", ["a", "b"])
def test_model_tiny_fp32_vs_reference(dev, golden_dir, name):
    """The stored state dict of model_tiny_a / model_tiny_b, floating tensors cast to fp32 and int8 left alone
    (tests/golden/gen_goldens_model.py:61-67).  tiny_a has intermediate_size 688 (K % 32 != 0): its down_proj stays on the generic
    kernel, every other projection takes the new route."""
    from onebit_amd.llama import OneBitLlamaConfig, OneBitLlamaForCausalLM
    z = np.load(os.path.join(golden_dir, f"model_tiny_{name}.npz"))
    kw = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg_")}
    cfg = OneBitLlamaConfig(**kw)
    model = OneBitLlamaForCausalLM(cfg, torch.float32)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")}
    model.load_state_dict({k: (v if v.dtype == torch.int8 else v.float()) for k, v in sd.items()})
    model = model.to(dev).eval()
    assert _all_projections_on_new_route(model, 8) == ({0, 2} if name == "a" else {2})
    ids = torch.from_numpy(z["input_ids"]).to(dev)
    with torch.no_grad():
        cache = model.new_cache(1, 32)
        lg = model(ids, cache)
        _model_check(f"model_tiny_{name}", z, "prefill_logits", lg.cpu().numpy())
        if "decode_logits_f32" in z.files:
            toks = torch.from_numpy(z["greedy_f32"]).to(dev)
            dec = np.concatenate([model(toks[:, i:i + 1], cache).cpu().numpy() for i in range(4)], axis=1)
            _model_check(f"model_tiny_{name}", z, "decode_logits", dec)
