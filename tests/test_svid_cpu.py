"""CPU-only checks of the SVID initialiser: the float64 restatement (tests/_svid_ref.py) reproduces the fixture recorded from
sklearn's own NMF (tests/golden/svid.npz) -- iteration counts exactly, vectors to the precision sklearn computed them in --,
``svid_init`` makes sklearn's draws bit for bit, the new C-ABI entry points exist in the header, the binding and the library,
choose their route without a device and reject bad arguments before any launch, and the Python surface fails loudly on CPU
tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _svid_ref
from onebit_amd import _lib
from onebit_amd import svid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVID_SYMBOLS = ["onebit_svid_workspace_bytes", "onebit_svid_route", "onebit_svid_iterate", "onebit_svid_emit"]
SHAPES = {(1, 8), (37, 72), (48, 64), (136, 344), (344, 136), (24, 2080)}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "svid.npz"))


def test_fixture_covers_the_cases_of_the_issue(golden):
    z, cases = golden, [str(c) for c in golden["cases"]]
    arrays = {c: z[f"{c}_A"] for c in cases}
    assert SHAPES <= {a.shape for a in arrays.values() if a.dtype == np.float32}
    assert any(a.dtype == np.float16 for a in arrays.values()) and any(a.dtype == np.float64 for a in arrays.values())
    assert any((a == 0).all() for a in arrays.values())                                             # the all-zero matrix
    some = lambda pred: any(pred(a) for a in arrays.values() if a.any())
    assert some(lambda a: ((a == 0).all(axis=1)).any()) and some(lambda a: ((a == 0).all(axis=0)).any())    # a zero row, a zero column
    assert some(lambda a: (np.signbit(a) & (a == 0)).any()) and some(lambda a: (~np.signbit(a) & (a == 0)).any())   # -0.0 and +0.0
    ratio = lambda v: np.sort(v)[-1] / np.median(v)
    assert some(lambda a: ratio(np.abs(a).mean(axis=1)) >= 8) and some(lambda a: ratio(np.abs(a).mean(axis=0)) >= 8)   # outliers
    for c in cases:                                  # the stopping rule sits a factor 2 from tol on both sides
        if int(z[f"{c}_n_iter"]) > 1:
            assert float(z[f"{c}_ratio_stop"]) <= 0.5e-4 and float(z[f"{c}_ratio_prev"]) >= 2e-4, c
        assert all(a.size <= 60000 for a in arrays.values())


def test_restatement_reproduces_sklearn(golden):
    z = golden
    worst32 = 0.0
    for c in (str(c) for c in z["cases"]):
        a = z[f"{c}_A"]
        w, h, n_iter, _ = _svid_ref.nmf_rank1(a)
        assert n_iter == int(z[f"{c}_n_iter"]), c
        gap = max(_svid_ref.max_rel(z[f"{c}_W"], w), _svid_ref.max_rel(z[f"{c}_H"], h))
        if a.dtype == np.float32:
            assert z[f"{c}_W"].dtype == np.float32 and gap <= 2e-6, (c, gap)
            worst32 = max(worst32, gap)
        else:
            assert z[f"{c}_W"].dtype == np.float64 and gap <= 1e-12, (c, gap)
        assert not np.isnan(w).any() and not np.isnan(h).any()
    assert worst32 == pytest.approx(float(z["fp32_gap"]), rel=1e-6)
    c = "allzero_16x24"                              # what the reference returns for the all-zero matrix: zeros after one iteration
    assert int(z[f"{c}_n_iter"]) == 1 and not z[f"{c}_W"].any() and not z[f"{c}_H"].any()
    # the model-level case: the same recipe on the seeded teacher
    sd = _svid_ref.teacher_arrays()
    for stem in _svid_ref.proj_keys():
        w, h, n_iter, _ = _svid_ref.nmf_rank1(sd[stem + ".weight"])
        assert n_iter == int(z[f"model/{stem}.n_iter"]), stem
        assert max(_svid_ref.max_rel(z[f"model/{stem}.weight_scale"], w), _svid_ref.max_rel(z[f"model/{stem}.input_factor"], h)) <= 2e-6, stem


def test_svid_init_makes_sklearns_draws_bit_for_bit(golden):
    z = golden
    for c in (str(c) for c in z["cases"]):
        a = z[f"{c}_A"]
        ct = np.float32 if a.dtype == np.float32 else np.float64
        N, K = a.shape
        w0, h0 = svid.svid_init(N, K, z[f"{c}_mean"], ct)
        assert w0.dtype == ct and h0.dtype == ct and w0.shape == (N,) and h0.shape == (K,)
        assert w0.tobytes() == z[f"{c}_w0"].tobytes() and h0.tobytes() == z[f"{c}_h0"].tobytes(), c
    w1, h1 = svid.svid_init(5, 8, 0.25, np.float32, random_state=1)
    w2, h2 = svid.svid_init(5, 8, 0.25, np.float32, random_state=0)
    assert not np.array_equal(h1, h2) and (h1 > 0).all() and (w1 > 0).all()


def test_symbols_in_header_binding_and_library():
    src = open(os.path.join(ROOT, "include", "onebit.h")).read()
    assert "#define ONEBIT_ABI_VERSION 10" in src
    assert f"#define ONEBIT_SVID_ONEPASS_MAX_K {_lib.SVID_ONEPASS_MAX_K}" in src and f"#define ONEBIT_SVID_STATS {_lib.SVID_STATS}" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(onebit_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for name in SVID_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.onebit_abi_version() == 10 and _lib.ABI_VERSION == 10


def test_route_needs_no_device():
    lib = _lib.load()
    bound = _lib.SVID_ONEPASS_MAX_K
    assert bound >= 13824
    for dt in (0, 1):
        assert lib.onebit_svid_route(4096, 11008, dt) == 1 and lib.onebit_svid_route(11008, 4096, dt) == 1
        assert lib.onebit_svid_route(5120, 13824, dt) == 1 and lib.onebit_svid_route(13824, 5120, dt) == 1
        assert lib.onebit_svid_route(1, 8, dt) == 1 and lib.onebit_svid_route(7, bound, dt) == 1
        assert lib.onebit_svid_route(7, bound + 8, dt) == 2 and lib.onebit_svid_route(4096, 32768, dt) == 2
    assert lib.onebit_svid_route(16, 12, 0) == -2 and lib.onebit_svid_route(16, 16, 5) == -4 and lib.onebit_svid_route(0, 16, 0) == -1


def test_argument_errors_without_gpu():
    lib = _lib.load()
    E_ARG, E_SHAPE, E_ALIGN, E_DTYPE, E_WSPACE = -1, -2, -3, -4, -5
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 63) & ~63
    N, K = 16, 64
    need = lib.onebit_svid_workspace_bytes(N, K, 1)
    assert 0 < need <= (1 << 16) - 64
    assert lib.onebit_svid_workspace_bytes(N, 12, 1) == 0 and lib.onebit_svid_workspace_bytes(N, K, 9) == 0
    big = _lib.SVID_ONEPASS_MAX_K + 8
    assert lib.onebit_svid_workspace_bytes(4096, 32768, 0) >= 4 * 32768            # the two-pass route's partials are covered
    it = lambda **k: lib.onebit_svid_iterate(k.get("A", a), k.get("dt", 1), k.get("lda", K), k.get("w", a), k.get("h", a), k.get("stats", a),
                                             k.get("ws", a), k.get("nws", need), k.get("N", N), k.get("K", K), k.get("route", 0), None)
    em = lambda **k: lib.onebit_svid_emit(k.get("A", a), k.get("dt", 1), k.get("lda", K), k.get("w", a), k.get("h", a), k.get("lat", a),
                                          k.get("ldt", 1), 0.01, k.get("packed", a), k.get("sums", a), k.get("ws", a), k.get("nws", need),
                                          k.get("N", N), k.get("K", K), None)
    for fn in (it, em):
        assert fn(K=12, lda=16) == E_SHAPE and fn(K=0) == E_ARG and fn(N=0) == E_ARG
        assert fn(A=None) == E_ARG
        assert b"null pointer" in lib.onebit_last_error()
        assert fn(dt=2) == E_DTYPE and fn(dt=-1) == E_DTYPE
        assert fn(lda=K - 8) == E_ARG and fn(lda=K + 4) == E_ALIGN and fn(A=a + 4) == E_ALIGN
        assert fn(nws=need - 4 if fn is it else 4) == E_WSPACE
        assert b"workspace" in lib.onebit_last_error()
        assert fn(ws=None) == E_ARG and fn(w=None) == E_ARG and fn(h=None) == E_ARG
    assert it(stats=None) == E_ARG and it(route=3) == E_ARG and it(route=-1) == E_ARG
    assert it(K=big, lda=big, route=1, nws=1 << 40) == E_ARG                       # the one-pass route forced beyond its bound
    assert b"one-pass" in lib.onebit_last_error()
    assert em(ldt=3) == E_DTYPE and em(lat=a + 8) == E_ALIGN
    assert em(lat=None, packed=None, sums=None, w=None, h=None, ws=None) == 0      # nothing asked for: nothing launched


def test_python_surface_fails_loudly_on_cpu():
    import onebit_amd
    for name in ("svid_init", "svid_decompose", "svid_start_layer", "build_start_state_dict", "build_inference_state_dict", "SvidResult"):
        assert getattr(onebit_amd, name) is getattr(svid, name)
    assert svid.SvidResult._fields == ("weight_scale", "input_factor", "n_iter", "rel_residual")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        svid.svid_decompose(torch.randn(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        svid.svid_start_layer(torch.randn(4, 8))
    sd = {"model.embed_tokens.weight": torch.randn(4, 8), "model.layers.0.self_attn.q_proj.weight": torch.randn(8, 8)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        svid.build_start_state_dict(sd, device="cpu")
    # only projection weights are decomposed: a dict without any is copied untouched, on any device
    plain = {"model.embed_tokens.weight": torch.randn(4, 8), "model.norm.weight": torch.ones(8), "lm_head.weight": torch.randn(4, 8)}
    out = svid.build_inference_state_dict(plain, device="cpu")
    assert list(out) == list(plain) and all(out[k] is plain[k] for k in plain)


def test_command_line_arguments_and_layout(tmp_path, capsys):
    """``python -m onebit_amd.svid`` on a teacher without projection weights (nothing to decompose, so no device is needed):
    the directory it writes is the one ``checkpoint.py`` reads -- config.json with the teacher's sizes and the student's
    model_type / architectures, pytorch_model.bin with the state dict"""
    import json
    from onebit_amd import checkpoint
    teacher = {"model.embed_tokens.weight": torch.randn(16, 8), "model.norm.weight": torch.ones(8), "lm_head.weight": torch.randn(16, 8)}
    cfg = {"model_type": "llama", "architectures": ["LlamaForCausalLM"], "vocab_size": 16, "hidden_size": 8, "intermediate_size": 24,
           "num_hidden_layers": 0, "num_attention_heads": 2, "rms_norm_eps": 1e-6, "bos_token_id": 1}
    tdir = tmp_path / "teacher"
    tdir.mkdir()
    (tdir / "config.json").write_text(json.dumps(cfg))
    torch.save(teacher, str(tdir / checkpoint.WEIGHTS_NAME))
    for flags, arch in (([], "BitLlamaForCausalLM"), (["--packed"], "BitLlamaForCausalLMInf")):
        out = tmp_path / ("out" + arch)
        assert svid.main([str(tdir), str(out), "--device", "cpu"] + flags) is None
        assert sorted(os.listdir(out)) == ["config.json", checkpoint.WEIGHTS_NAME]
        raw = json.loads((out / "config.json").read_text())
        assert raw["model_type"] == "bitllama" and raw["architectures"] == [arch]
        assert {k: raw[k] for k in cfg if k not in ("model_type", "architectures")} == {k: v for k, v in cfg.items() if k not in ("model_type", "architectures")}
        read = checkpoint.config_from_json(str(out / "config.json"))
        assert (read.vocab_size, read.hidden_size, read.intermediate_size, read.num_attention_heads) == (16, 8, 24, 2)
        sd = torch.load(str(out / checkpoint.WEIGHTS_NAME), map_location="cpu", weights_only=True)
        assert list(sd) == list(teacher) and all(torch.equal(sd[k], teacher[k]) for k in teacher)
    for argv in ([], [str(tdir)], [str(tdir), str(tmp_path / "o"), "--no-such-flag"]):
        with pytest.raises(SystemExit):
            svid.main(argv)
    capsys.readouterr()
    with pytest.raises(FileNotFoundError):
        svid.main([str(tmp_path / "missing"), str(tmp_path / "o")])
