"""GPU checks of the SVID initialiser (onebit_amd/svid.py, csrc/ob_svid.h) against the float64 restatement (tests/_svid_ref.py)
and the fixture recorded from sklearn's NMF (tests/golden/svid.npz).

The tolerance: ``BAR = 4 x fp32_gap``, where ``fp32_gap`` (recorded by the generator) is the largest relative gap (max element)
between sklearn's own fp32 result and the float64 restatement at the same iteration count -- the reference's rounding noise.
The kernels sum in another order than BLAS, both O(sqrt(n)) 2^-24 walks; one dropped or doubled element moves a vector by
>= 1 / K ~ 5e-4 at these sizes, orders of magnitude above the bar.  Measured errors are printed and, when OB_SVID_PARITY_LOG
names a file, appended to it (the source of the figures in profiles/svid.txt)."""
import os

import numpy as np
import pytest
import torch

import _svid_ref
from onebit_amd import _lib, svid

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "svid.npz"))


@pytest.fixture(scope="module")
def bar(golden):
    return 4.0 * float(golden["fp32_gap"])


def _cases(z):
    return [str(c) for c in z["cases"]]


def _gpu_input(a):
    """the matrix as the GPU takes it: float64 storage of fp32 values is given as fp32"""
    return torch.from_numpy(a.astype(np.float32) if a.dtype == np.float64 else a).to(DEV)


_REF = {}


def _ref(z, c):
    """float64 restatement on the GPU's input at the golden's iteration count, computed once per case"""
    if c not in _REF:
        a = z[f"{c}_A"]
        a = a.astype(np.float32) if a.dtype == np.float64 else a
        _REF[c] = _svid_ref.nmf_rank1(a, n_iter=int(z[f"{c}_n_iter"]))[:2]
    return _REF[c]


def _log(line):
    print(line)
    path = os.environ.get("OB_SVID_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _err(res, w, h):
    return max(_svid_ref.max_rel(res.weight_scale.cpu().numpy(), w), _svid_ref.max_rel(res.input_factor.cpu().numpy(), h))


@pytest.mark.parametrize("route", [1, 2])
def test_fixed_iteration_count_matches_restatement(golden, bar, route):
    z = golden
    for c in _cases(z):
        w, h = _ref(z, c)
        res = svid.svid_decompose(_gpu_input(z[f"{c}_A"]), n_iter=int(z[f"{c}_n_iter"]), route=route)
        e = _err(res, w, h)
        _log(f"fixed n_iter  route {route}  {c:16s} max rel err {e:.3e}  bar {bar:.3e}")
        assert res.n_iter == int(z[f"{c}_n_iter"]) and res.weight_scale.dtype == torch.float32
        assert e <= bar, (c, route, e, bar)


def test_stopping_rule_reproduces_sklearns_iteration_count(golden, bar):
    z = golden
    for c in _cases(z):
        for route in (0, 2):
            res = svid.svid_decompose(_gpu_input(z[f"{c}_A"]), route=route)
            assert res.n_iter == int(z[f"{c}_n_iter"]), (c, route, res.n_iter)
        w, h = _ref(z, c)
        assert _err(res, w, h) <= bar, c


def test_layout_edges(golden, bar):
    z = golden
    for c in ("zeros_37x72", "outcol_136x344", "wide_24x2080"):          # partial chunk patterns; N no multiple of the band height
        a = z[f"{c}_A"]
        n_iter = int(z[f"{c}_n_iter"])
        w, h = _ref(z, c)
        N, K = a.shape
        wide = torch.full((N, K + 24), float("nan"), dtype=torch.float32, device=DEV)      # lda > K: what lies beyond is never read
        wide[:, :K] = torch.from_numpy(a).to(DEV)
        view = wide[:, :K]
        assert view.stride(0) == K + 24 and not view.is_contiguous()
        for route in (1, 2):
            res = svid.svid_decompose(view, n_iter=n_iter, route=route)
            e = _err(res, w, h)
            _log(f"strided view  route {route}  {c:16s} max rel err {e:.3e}  bar {bar:.3e}")
            assert e <= bar, (c, route, e)
            same = svid.svid_decompose(torch.from_numpy(a).to(DEV), n_iter=n_iter, route=route)
            assert torch.equal(same.weight_scale, res.weight_scale) and torch.equal(same.input_factor, res.input_factor)
    # fp16 A against the same values widened to fp32: the kernels' arithmetic is the same fp32 (the draws differ in rounding only)
    c = "half_40x136"
    a16 = z[f"{c}_A"]
    n_iter = int(z[f"{c}_n_iter"])
    for route in (1, 2):
        r16 = svid.svid_decompose(torch.from_numpy(a16).to(DEV), n_iter=n_iter, route=route)
        r32 = svid.svid_decompose(torch.from_numpy(a16.astype(np.float32)).to(DEV), n_iter=n_iter, route=route)
        e = _err(r16, r32.weight_scale.cpu().numpy(), r32.input_factor.cpu().numpy())
        _log(f"fp16 vs fp32  route {route}  {c:16s} max rel gap {e:.3e}  bar {bar:.3e}")
        assert e <= bar, (route, e)


@pytest.mark.parametrize("N,K,dt", [(6, 4104, torch.float16), (7, 4104, torch.float32), (5, 8200, torch.float16), (3, 8200, torch.float32),
                                    (9, 13824, torch.float16), (3, 16392, torch.float16), (2, 16392, torch.float32)])
def test_wide_rows_take_the_other_kernel_forms(bar, N, K, dt):
    """K beyond 4096 / 8192 switches the one-pass kernel to 1024 threads with one / two chunks per thread (a partial second
    chunk at 8200 and 13824), K beyond the one-pass bound leaves the two-pass route alone; few rows keep it quick.  No sklearn
    fixture at these widths: the float64 restatement (pinned to sklearn by the fixture) at a fixed iteration count."""
    lib = _lib.load()
    rng = np.random.RandomState(K + N)
    a = (0.02 * rng.standard_normal((N, K)) * np.exp(0.4 * rng.standard_normal((1, K)))).astype(np.float32)
    a = a.astype(np.float16) if dt == torch.float16 else a
    a[:, 5] = 0.0
    auto = lib.onebit_svid_route(N, K, 0)
    assert auto == (1 if K <= _lib.SVID_ONEPASS_MAX_K else 2)
    w, h, _, _ = _svid_ref.nmf_rank1(a, n_iter=4)
    at = torch.from_numpy(a).to(DEV)
    for route in ((1, 2) if auto == 1 else (0,)):
        res = svid.svid_decompose(at, n_iter=4, route=route)
        e = _err(res, w, h)
        _log(f"wide rows     route {route or auto}  {N}x{K} {str(dt)[6:]:8s} max rel err {e:.3e}  bar {bar:.3e}")
        assert e <= bar, (route, e, bar)
        assert float(res.input_factor[5]) == 0.0
        want = _svid_ref.rel_residual(a, res.weight_scale.double().cpu().numpy(), res.input_factor.double().cpu().numpy())
        assert abs(res.rel_residual - want) <= 1e-5 * want
    if auto == 2:
        with pytest.raises(ValueError, match="one-pass"):
            svid.svid_decompose(at, n_iter=1, route=1)


def _emit(a, w, h, latent=None, packed=None, sums=None, scale=0.01):
    lib = _lib.load()
    N, K = a.shape
    code = 0 if a.dtype == torch.float16 else 1
    nws = lib.onebit_svid_workspace_bytes(N, K, code)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    rc = lib.onebit_svid_emit(a.data_ptr(), code, a.stride(0), w.data_ptr(), h.data_ptr(), None if latent is None else latent.data_ptr(),
                              0 if latent is None or latent.dtype == torch.float16 else 1, scale, None if packed is None else packed.data_ptr(),
                              None if sums is None else sums.data_ptr(), ws.data_ptr(), nws, N, K, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.onebit_last_error()


def test_emit_outputs(golden):
    from onebit_amd import pack_signs
    z = golden
    for c, dt in (("zeros_37x72", torch.float32), ("outcol_136x344", torch.float32), ("half_40x136", torch.float16)):
        a = torch.from_numpy(z[f"{c}_A"]).to(DEV)
        assert a.dtype == dt
        N, K = a.shape
        res = svid.svid_decompose(a)
        w, h = res.weight_scale, res.input_factor
        want = _svid_ref.rel_residual(z[f"{c}_A"], w.double().cpu().numpy(), h.double().cpu().numpy())
        _log(f"rel_residual  {c:16s} gpu {res.rel_residual:.8f}  float64 {want:.8f}  rel gap {abs(res.rel_residual - want) / want:.2e}")
        assert abs(res.rel_residual - want) <= 1e-5 * want
        for ldt in (torch.float16, torch.float32):
            latent = torch.full((N, K), 7.0, dtype=ldt, device=DEV)
            packed = torch.full((N, K // 8), 0x55, dtype=torch.int8, device=DEV)
            sums = torch.zeros(2, device=DEV)
            _emit(a, w, h, latent, packed, sums)
            ref_latent = torch.sign(a.to(ldt)) * 0.01
            assert torch.equal(latent.view(torch.int16 if ldt == torch.float16 else torch.int32),
                               ref_latent.view(torch.int16 if ldt == torch.float16 else torch.int32)), (c, ldt)      # bit for bit, zeros included
            assert torch.equal(packed, pack_signs(a)), c
            assert abs(float(torch.sqrt(sums[0] / sums[1])) - want) <= 1e-5 * want
            # one output only: the other buffer stays untouched
            lat2 = torch.full((N, K), 7.0, dtype=ldt, device=DEV)
            pk2 = torch.full((N, K // 8), 0x55, dtype=torch.int8, device=DEV)
            _emit(a, w, h, latent=lat2)
            assert torch.equal(lat2, latent) and bool((pk2 == 0x55).all())
            lat3 = torch.full((N, K), 7.0, dtype=ldt, device=DEV)
            _emit(a, w, h, packed=pk2)
            assert torch.equal(pk2, packed) and bool((lat3 == 7.0).all())
    lat, ws_, hs_ = svid.svid_start_layer(a)
    assert lat.dtype == a.dtype and torch.equal(lat, torch.sign(a) * 0.01)
    assert torch.equal(ws_, w) and torch.equal(hs_, h)
    assert svid.svid_start_layer(a, latent_dtype=torch.float32)[0].dtype == torch.float32


def test_edge_inputs(golden):
    z = golden
    c = "allzero_16x24"
    res = svid.svid_decompose(_gpu_input(z[f"{c}_A"]))
    assert res.n_iter == int(z[f"{c}_n_iter"]) == 1 and res.rel_residual == 0.0
    assert np.array_equal(res.weight_scale.cpu().numpy(), z[f"{c}_W"]) and np.array_equal(res.input_factor.cpu().numpy(), z[f"{c}_H"])
    for c, row in (("zeros_37x72", 11), ("tall_344x136", 300)):           # an all-zero row: its scale is exactly 0
        for route in (1, 2):
            res = svid.svid_decompose(_gpu_input(z[f"{c}_A"]), route=route)
            assert float(res.weight_scale[row]) == 0.0 and int((res.weight_scale == 0).sum()) == 1
            assert bool(torch.isfinite(res.weight_scale).all()) and bool(torch.isfinite(res.input_factor).all())
    res = svid.svid_decompose(_gpu_input(z["outcol_136x344_A"]))
    assert float(res.input_factor[200]) == 0.0                              # and an all-zero column
    for bad in (float("nan"), float("inf"), -float("inf")):
        for dt in (torch.float32, torch.float16):
            a = torch.from_numpy(z["outrow_48x64_A"]).to(DEV).to(dt)
            a[7, 9] = bad
            with pytest.raises(ValueError, match="NaN or infinity"):
                svid.svid_decompose(a)
            with pytest.raises(ValueError, match="NaN or infinity"):
                svid.svid_start_layer(a)
            sd = {"model.layers.0.mlp.up_proj.weight": a.cpu()}
            with pytest.raises(ValueError, match="NaN or infinity"):
                svid.build_start_state_dict(sd)
            assert list(sd) == ["model.layers.0.mlp.up_proj.weight"]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_iterate_reports_non_finite_input_and_writes_only_its_outputs(golden, bad):
    """the C entry point itself on a matrix with one NaN / infinity and finite w, h: the violation in stats[0] comes back
    non-finite (what ``svid_decompose`` turns into ValueError), A is not written, and nothing lands outside w, h, stats and
    the workspace -- each of those sits between guard words in one buffer"""
    lib = _lib.load()
    a = torch.from_numpy(golden["outrow_48x64_A"]).to(DEV)
    a[7, 9] = bad
    before = a.clone()
    N, K = a.shape
    nws = lib.onebit_svid_workspace_bytes(N, K, 1)
    assert nws % 4 == 0
    G = 64                                             # guard floats: 256 bytes keep every slice 16-byte aligned
    sizes = [N, K, _lib.SVID_STATS + (-_lib.SVID_STATS) % 4, nws // 4 + (-(nws // 4)) % 4]
    w0, h0 = svid.svid_init(N, K, 0.02, np.float32)
    for route in (1, 2):
        buf = torch.full((G + sum(n + G for n in sizes),), -7.0, device=DEV)
        offs = np.cumsum([G] + [n + G for n in sizes[:-1]])
        w, h, stats, ws = (buf[o:o + n] for o, n in zip(offs, sizes))
        w.copy_(torch.from_numpy(w0))
        h.copy_(torch.from_numpy(h0))
        rc = lib.onebit_svid_iterate(a.data_ptr(), 1, a.stride(0), w.data_ptr(), h.data_ptr(), stats.data_ptr(), ws.data_ptr(), nws,
                                     N, K, route, None)
        torch.cuda.synchronize()
        assert rc == 0, lib.onebit_last_error()
        assert not np.isfinite(float(stats[0])), (route, float(stats[0]))
        guards = torch.ones_like(buf, dtype=torch.bool)
        for o, n in zip(offs, sizes):
            guards[o:o + n] = False
        assert bool((buf[guards] == -7.0).all()), route
        assert torch.equal(a.view(torch.int32), before.view(torch.int32))
        assert bool(torch.isfinite(w[torch.arange(N, device=DEV) != 7]).all())         # the other rows' scales stay finite


@pytest.mark.parametrize("dt,strided", [(torch.float16, False), (torch.float32, False), (torch.float16, True)])
def test_no_copy_of_the_matrix_is_made(dt, strided):
    """Peak device memory of one ``svid_decompose`` above what is held before it: the workspace, the vectors and the
    statistics -- less than the matrix itself, so neither ``|A|`` nor a widened copy of ``A`` (2 to 4 times its bytes) exists
    at any point, the reduction behind ``mean |A|`` for the draws included."""
    N, K = 512, 1024
    g = torch.Generator(device=DEV).manual_seed(5)
    buf = (0.02 * torch.randn(N, K + 64, generator=g, device=DEV)).to(dt)
    a = buf[:, :K] if strided else buf[:, :K].contiguous()
    del buf
    svid.svid_decompose(a, n_iter=1)                   # the library, its kernels and the allocator's pools are in place
    nws = _lib.load().onebit_svid_workspace_bytes(N, K, 0 if dt == torch.float16 else 1)
    allowed = nws + 32 * (N + K) + (64 << 10)          # w, h, their host-side staging, row sums in fp32 and fp64; 512-byte rounding
    assert allowed < N * K * a.element_size()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    res = svid.svid_decompose(a)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - held
    _log(f"peak memory   {N}x{K} {str(dt)[6:]:8s} strided {strided!s:5s} extra {extra} bytes  allowed {allowed}  matrix {N * K * a.element_size()}")
    assert res.n_iter >= 2 and extra <= allowed, (extra, allowed)


def test_two_runs_are_bit_identical(golden):
    z = golden
    for c in ("tall_344x136", "wide_24x2080", "half_40x136"):
        a = _gpu_input(z[f"{c}_A"])
        for route in (1, 2):
            r1, r2 = svid.svid_decompose(a, route=route), svid.svid_decompose(a, route=route)
            assert torch.equal(r1.weight_scale, r2.weight_scale) and torch.equal(r1.input_factor, r2.input_factor)
            assert r1.n_iter == r2.n_iter and r1.rel_residual == r2.rel_residual


@pytest.fixture(scope="module")
def teacher():
    return {k: torch.from_numpy(v) for k, v in _svid_ref.teacher_arrays().items()}


_MODEL_N_ITER = {}


@pytest.fixture(scope="module")
def start_sd(teacher):
    return svid.build_start_state_dict(teacher, progress=lambda done, total, stem, n_iter, rel: _MODEL_N_ITER.__setitem__(stem, n_iter))


def test_model_start_state_dict_matches_reference_recipe(golden, bar, teacher, start_sd):
    z = golden
    assert list(start_sd) == [str(k) for k in z["model_keys"]]
    assert [str(v.dtype).replace("torch.", "") for v in start_sd.values()] == [str(d) for d in z["model_dtypes"]]
    worst = 0.0
    for stem in _svid_ref.proj_keys():
        e = max(_svid_ref.max_rel(start_sd[stem + ".weight_scale"].numpy(), z[f"model/{stem}.weight_scale"]),
                _svid_ref.max_rel(start_sd[stem + ".input_factor"].numpy(), z[f"model/{stem}.input_factor"]))
        worst = max(worst, e)
        assert e <= bar, (stem, e, bar)
        assert _MODEL_N_ITER[stem] == int(z[f"model/{stem}.n_iter"]), stem             # the stopping rule, projection by projection
        assert torch.equal(start_sd[stem + ".weight"], torch.sign(teacher[stem + ".weight"]) * 0.01)
    _log(f"model level   14 projections    max rel err vs sklearn fp32 {worst:.3e}  bar {bar:.3e}")
    for k, v in teacher.items():
        if k[:-len(".weight")] not in _svid_ref.proj_keys():
            assert start_sd[k] is v


def test_model_packed_equals_converted_and_runs(teacher, start_sd):
    from onebit_amd import BitLinearInf
    from onebit_amd.checkpoint import convert_train_state_dict
    from onebit_amd.llama import OneBitLlamaConfig, OneBitLlamaForCausalLM
    from onebit_amd.train import BitLinear
    packed_sd = svid.build_inference_state_dict(teacher)
    conv = convert_train_state_dict(start_sd)
    assert list(packed_sd) == list(conv)
    for k in conv:
        assert packed_sd[k].dtype == conv[k].dtype and torch.equal(packed_sd[k], conv[k]), k
    R = _svid_ref
    cfg = OneBitLlamaConfig(vocab_size=R.MODEL_VOCAB, hidden_size=R.MODEL_HIDDEN, intermediate_size=R.MODEL_INTER,
                            num_hidden_layers=R.MODEL_LAYERS, num_attention_heads=R.MODEL_HEADS, max_position_embeddings=64)
    model = OneBitLlamaForCausalLM(cfg, torch.float16)
    model.load_state_dict({k: (v if not v.is_floating_point() else v.half()) for k, v in packed_sd.items()})
    model = model.to(DEV).eval()
    ids = torch.from_numpy(np.random.RandomState(3).randint(0, R.MODEL_VOCAB, size=(1, 8))).to(DEV)
    with torch.no_grad():
        logits = model(ids)
    assert logits.shape[-1] == R.MODEL_VOCAB and bool(torch.isfinite(logits.float()).all())
    # the latent layer (train.BitLinear) and the packed layer (BitLinearInf) agree: test_gpu_train.py's train-vs-inference tolerance
    stem = "model.layers.1.mlp.down_proj"
    K, N = R.MODEL_INTER, R.MODEL_HIDDEN
    m = BitLinear(K, N).to(DEV)
    m.load_state_dict({n: start_sd[f"{stem}.{n}"] for n in ("weight", "weight_scale", "input_factor")})
    assert int((m.weight == 0).sum()) == 0
    inf = BitLinearInf(K, N, dtype=torch.float32).to(DEV)
    inf.load_state_dict({n: packed_sd[f"{stem}.{n}"] for n in ("weight", "weight_scale", "input_factor")})
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((9, K)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        assert float((m(x) - inf(x)).abs().max()) <= 2e-4
