"""CPU-only checks of the knowledge-distillation loss: the float64 restatement (tests/_kd_ref.py) reproduces the fixture
recorded from the reference's own ``KDTrainer.compute_loss`` (tests/golden/kd_loss.npz), the new C-ABI entry points exist in
the header, the binding and the library and reject bad arguments before any launch, and the Python surface fails loudly
where it must (CPU tensors, the attention-weight term)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _kd_ref
from onebit_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_SYMBOLS = ["onebit_kd_token_forward", "onebit_kd_token_backward", "onebit_kd_hidden_forward", "onebit_kd_hidden_backward"]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def test_restatement_reproduces_reference_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "kd_loss.npz"))
    labels = torch.from_numpy(z["labels"])
    assert (z["labels"] == -100).sum() >= 2 and z["s_logits"].shape == (2, 5, 320)
    n_states = 4
    for c in (0, 1):
        alpha, beta, scale = float(z[f"case{c}_alpha"]), float(z[f"case{c}_beta"]), float(z[f"case{c}_scale"])
        s = _kd_ref.to64(torch.from_numpy(z["s_logits"]))
        t = torch.from_numpy(z["t_logits"]).double()
        sh = [_kd_ref.to64(torch.from_numpy(z[f"s_h{i}"])) for i in range(n_states)]
        th = [torch.from_numpy(z[f"t_h{i}"]).double() for i in range(n_states)]
        loss = _kd_ref.kd_loss(s, t, labels, sh, th, None, kd_alpha=alpha, kd_beta=beta, kd_loss_scale=scale)
        loss.backward()
        assert abs(float(loss.detach()) - float(z[f"case{c}_loss"])) <= 1e-12 * abs(float(z[f"case{c}_loss"]))
        kl = _kd_ref.kl_batchmean(s.detach(), t)
        assert abs(float(kl) - float(z[f"case{c}_kl"])) <= 1e-12 * abs(float(z[f"case{c}_kl"]))
        assert _rel(s.grad.numpy(), z[f"case{c}_g_logits"]) <= 1e-12
        for i in range(n_states - 1):
            assert _rel(sh[i].grad.numpy(), z[f"case{c}_g_h{i}"]) <= 1e-12, i
        # the loop quirk: n_layers entries of n_layers + 1 states, so the last one is never read
        assert sh[n_states - 1].grad is None and f"case{c}_g_h{n_states - 1}" not in z.files
    # batchmean divides by B, not by B * S: the row-mean is S times smaller
    s, t = torch.from_numpy(z["s_logits"]).double(), torch.from_numpy(z["t_logits"]).double()
    rows = (torch.softmax(t, -1) * (torch.log_softmax(t, -1) - torch.log_softmax(s, -1))).sum(-1)
    assert abs(float(rows.sum() / 2) - float(z["case0_kl"])) <= 1e-12 * float(z["case0_kl"])


def test_symbols_in_header_binding_and_library():
    src = open(os.path.join(ROOT, "include", "onebit.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(onebit_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for name in KD_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.onebit_abi_version() == 10 and _lib.ABI_VERSION == 10
    assert "#define ONEBIT_ABI_VERSION 10" in open(os.path.join(ROOT, "include", "onebit.h")).read()


def test_argument_errors_without_gpu():
    lib = _lib.load()
    E_ARG, E_SHAPE, E_ALIGN, E_DTYPE = -1, -2, -3, -4
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) & ~63
    tf = lambda **k: lib.onebit_kd_token_forward(k.get("s", a), k.get("t", a), k.get("lab", a), k.get("stats", a), k.get("sums", a),
                                                 k.get("T", 3), k.get("V", 8), k.get("dt", 1), -100, None)
    tb = lambda **k: lib.onebit_kd_token_backward(k.get("s", a), k.get("t", a), k.get("lab", a), k.get("stats", a), k.get("coef", a),
                                                  k.get("g", a), k.get("T", 3), k.get("V", 8), k.get("dt", 1), -100, None)
    hf = lambda **k: lib.onebit_kd_hidden_forward(k.get("s", a), k.get("t", a), k.get("stats", a), k.get("sums", a),
                                                  k.get("T", 3), k.get("H", 8), k.get("dt", 0), None)
    hb = lambda **k: lib.onebit_kd_hidden_backward(k.get("s", a), k.get("t", a), k.get("stats", a), k.get("coef", a), k.get("g", a),
                                                   k.get("T", 3), k.get("H", 8), k.get("dt", 0), None)
    for fn in (tf, tb, hf, hb):
        assert fn(s=None) == E_ARG and fn(stats=None) == E_ARG
        assert b"null pointer" in lib.onebit_last_error()
        assert fn(dt=2) == E_DTYPE and fn(dt=-1) == E_DTYPE
        assert fn(T=0) == 0
        assert fn(T=0, s=None, stats=None) == 0            # nothing to do: nothing is dereferenced
        assert fn(T=-1) == E_ARG
    assert tf(V=0) == E_SHAPE and tb(V=-5) == E_SHAPE and hf(H=0) == E_SHAPE and hb(H=-1) == E_SHAPE
    assert hf(t=None) == E_ARG and hb(t=None) == E_ARG       # (the token loss's teacher is nullable: the KL term switched off)
    assert tf(sums=None) == E_ARG and hf(sums=None) == E_ARG
    assert tb(coef=None) == E_ARG and tb(g=None) == E_ARG and hb(coef=None) == E_ARG and hb(g=None) == E_ARG
    assert hf(stats=a + 4) == E_ALIGN and hb(stats=a + 4) == E_ALIGN


def test_python_surface_fails_loudly_on_cpu():
    import onebit_amd
    from onebit_amd.kd import KDLoss, kd_hidden_loss, kd_token_loss
    assert onebit_amd.KDLoss is KDLoss and onebit_amd.kd_token_loss is kd_token_loss and onebit_amd.kd_hidden_loss is kd_hidden_loss
    m = KDLoss()
    assert (m.kd_alpha, m.kd_beta, m.kd_loss_scale, m.kd_gamma) == (0.8, 0.0, 1.0, 0.0)     # hparams/model_args.py:81-100
    with pytest.raises(NotImplementedError, match="attention"):
        KDLoss(kd_gamma=1)
    s, t = torch.randn(2, 3, 8), torch.randn(2, 3, 8)
    labels = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kd_token_loss(s, t, labels, kd_alpha=0.8, kd_loss_scale=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kd_hidden_loss([torch.randn(4, 8)], [torch.randn(4, 8)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(s, t, labels)
