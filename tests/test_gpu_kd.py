"""Knowledge-distillation loss on the GPU (onebit_amd/kd.py -> onebit_kd_* HIP kernels, csrc/ob_kd.h) against the fixture
recorded from the reference's ``KDTrainer.compute_loss`` (tests/golden/kd_loss.npz) and, at other shapes, against the float64
restatement that fixture pins (tests/_kd_ref.py, evaluated on the CPU on exactly the device's fp16 / fp32 input values).

Bars.  loss: ``|loss - ref| <= 2e-5 |ref| + 2 (T/B) ulp32(max|logit|)`` -- the second term is the one rounding of each row's
lse, which no fp32 evaluation avoids (T/B rows per unit of batchmean).  Gradients: rel-L2 <= 2e-4 in fp32, <= 2e-3 in fp16
(the bars of test_gpu_train.py; fp16 rounding of the exact gradient alone is 2.3e-4).  The hidden-state loss has no lse, so
its loss bar is the relative term alone.

Shapes: those the kernels' paths divide at -- rows of <= 8192 elements (256 threads), <= 32768 (1024 threads, the row in
registers), longer (walked in chunks); pitches that keep groups of four aligned and pitches that do not (32001, 32003, H = 99).
"""
import math
import os

import numpy as np
import pytest
import torch

import _kd_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_BAR = {torch.float32: 2e-4, torch.float16: 2e-3}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


def _loss_bar(ref, S, *logits):
    m = max(float(x[torch.isfinite(x)].abs().max()) for x in logits)
    return 2e-5 * abs(ref) + 2 * S * _ulp32(m)


def _check_loss(got, ref, bar, what):
    got, ref = float(got.detach() if torch.is_tensor(got) else got), float(ref.detach() if torch.is_tensor(ref) else ref)
    print(f"{what}: got {got!r} ref {ref!r} |diff| {abs(got - ref):.3e} bar {bar:.3e}")
    if math.isnan(ref):
        assert math.isnan(got), what
    else:
        assert abs(got - ref) <= bar, what


def _make(B, S, V, dtype, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    s = (scale * torch.randn(B, S, V, generator=g)).to(dtype)
    t = (scale * torch.randn(B, S, V, generator=g)).to(dtype)          # drawn independently: KL is O(1) per row
    labels = torch.randint(0, V, (B, S), generator=g)
    if S > 2:
        labels[0, 1] = -100
    return s, t, labels


def _token_case(s, t, labels, alpha, scale, what, check_grad=True):
    """Run kd_token_loss on the device and the restatement in float64 on the same values; assert the bars; return both."""
    from onebit_amd.kd import kd_token_loss
    B, S, V = s.shape
    sd = s.to(DEV).requires_grad_(True)
    loss, kl, ce = kd_token_loss(sd, t.to(DEV), None if labels is None else labels.to(DEV), kd_alpha=alpha, kd_loss_scale=scale)
    assert loss.dtype == torch.float32 and loss.shape == () and not kl.requires_grad and not ce.requires_grad
    s64 = _kd_ref.to64(s)
    rloss, rkl, rce = _kd_ref.token_loss(s64, t.double(), labels, alpha, scale)
    _check_loss(loss, rloss, _loss_bar(float(rloss), S, s.float(), t.float()), what + " loss")
    _check_loss(kl, rkl, _loss_bar(float(rkl), S, s.float(), t.float()), what + " kl")
    if rce is not None:
        _check_loss(ce, rce, _loss_bar(float(rce), 1, s.float()), what + " ce")
    if check_grad:
        loss.backward()
        assert sd.grad.dtype == s.dtype and sd.grad.shape == s.shape
        rloss.backward()
        r = _rel(sd.grad, s64.grad)
        print(f"{what}: grad rel-L2 {r:.3e}")
        assert torch.isfinite(sd.grad).all() and r <= GRAD_BAR[s.dtype], what
    return sd, s64, loss


def test_fixture_loss_and_gradients(golden_dir):
    from onebit_amd.kd import KDLoss, kd_token_loss
    z = np.load(os.path.join(golden_dir, "kd_loss.npz"))
    labels = torch.from_numpy(z["labels"]).to(DEV)
    S = z["s_logits"].shape[1]
    for c in (0, 1):
        alpha, beta, scale = float(z[f"case{c}_alpha"]), float(z[f"case{c}_beta"]), float(z[f"case{c}_scale"])
        s = torch.from_numpy(z["s_logits"]).to(DEV).requires_grad_(True)
        t = torch.from_numpy(z["t_logits"]).to(DEV)
        sh = [torch.from_numpy(z[f"s_h{i}"]).to(DEV).requires_grad_(True) for i in range(4)]
        th = [torch.from_numpy(z[f"t_h{i}"]).to(DEV) for i in range(4)]
        loss = KDLoss(kd_alpha=alpha, kd_beta=beta, kd_loss_scale=scale)(s, t, labels, tuple(sh), tuple(th))
        bar = _loss_bar(float(z[f"case{c}_loss"]), S, s.detach(), t)
        _check_loss(loss, z[f"case{c}_loss"], bar, f"fixture case {c} loss")
        _, kl, _ = kd_token_loss(s.detach(), t, labels, kd_alpha=alpha, kd_loss_scale=scale)
        _check_loss(kl, z[f"case{c}_kl"], _loss_bar(float(z[f"case{c}_kl"]), S, s.detach(), t), f"fixture case {c} kl")
        loss.backward()
        assert _rel(s.grad, torch.from_numpy(z[f"case{c}_g_logits"])) <= 2e-4
        for i in range(3):
            assert _rel(sh[i].grad, torch.from_numpy(z[f"case{c}_g_h{i}"])) <= 2e-4, i
        assert sh[3].grad is None                          # the reference's loop never reads the last hidden state


@pytest.mark.parametrize("B,S,V,dtype", [
    (1, 1, 8, torch.float32), (3, 7, 1000, torch.float32), (2, 3, 32000, torch.float32), (1, 4, 32003, torch.float32),
    (2, 5, 320, torch.float16), (1, 3, 32001, torch.float16),
    # the path boundaries: last row length of the 256-thread kernel and the first of the 1024-thread one, rows longer than
    # the registers hold (walked in chunks) with an aligned and an unaligned pitch
    (1, 2, 8192, torch.float32), (1, 2, 8196, torch.float32), (1, 2, 40001, torch.float32), (1, 2, 33000, torch.float16),
])
def test_token_loss_shapes_vs_restatement(B, S, V, dtype):
    s, t, labels = _make(B, S, V, dtype, seed=B + S + V)
    _token_case(s, t, labels, 0.8, 1.0, f"{(B, S, V)} {dtype}")


def test_teacher_minus_inf_entries_add_nothing():
    s, t, labels = _make(1, 3, 1000, torch.float32, seed=5)
    t[0, 1, ::7] = -math.inf
    t[0, 2, 3] = -math.inf
    _, _, loss = _token_case(s, t, labels, 0.8, 1.0, "teacher -inf")
    assert math.isfinite(float(loss))


@pytest.mark.parametrize("dtype,big", [(torch.float16, 6e4), (torch.float32, 1e4)])
def test_extreme_logits_do_not_overflow(dtype, big):
    s, t, labels = _make(2, 3, 1000, dtype, seed=6)
    g = torch.Generator().manual_seed(7)
    s[0, 1] = torch.where(torch.rand(1000, generator=g) < 0.5, -big, big).to(dtype)
    t[0, 1] = torch.where(torch.rand(1000, generator=g) < 0.5, -big, big).to(dtype)
    t[1, 0] = s[1, 0] = torch.where(torch.rand(1000, generator=g) < 0.5, -big, big).to(dtype)
    sd, _, loss = _token_case(s, t, labels, 0.8, 1.0, f"extreme {dtype}")
    assert math.isfinite(float(loss)) and torch.isfinite(sd.grad).all()


def test_all_labels_ignored_none_and_switches():
    from onebit_amd.kd import kd_token_loss
    s, t, labels = _make(2, 4, 320, torch.float32, seed=8)
    # every label ignored: CE is NaN as torch's mean over nothing; with kd_alpha = 1 the KL and its gradient stay finite
    ign = torch.full_like(labels, -100)
    sd = s.to(DEV).requires_grad_(True)
    loss, kl, ce = kd_token_loss(sd, t.to(DEV), ign.to(DEV), kd_alpha=1.0, kd_loss_scale=0.5)
    assert math.isnan(float(ce)) and math.isfinite(float(kl))
    s64 = _kd_ref.to64(s)
    rloss, rkl, rce = _kd_ref.token_loss(s64, t.double(), ign, 1.0, 0.5)
    assert math.isnan(float(rce)) and math.isnan(float(rloss)) == math.isnan(float(loss))
    _check_loss(kl, rkl, _loss_bar(float(rkl), 4, s, t), "ignored kl")
    loss.backward()
    (0.5 * rkl).backward()
    assert torch.isfinite(sd.grad).all() and _rel(sd.grad, s64.grad) <= 2e-4
    # labels=None drops the CE term, kd_loss_scale = 0 the KL term
    _token_case(s, t, None, 0.8, 1.0, "labels=None")
    sd0, _, loss0 = _token_case(s, t, labels, 0.8, 0.0, "scale=0")
    _, kl0, _ = kd_token_loss(sd0.detach(), t.to(DEV), labels.to(DEV), kd_alpha=0.8, kd_loss_scale=0.0)
    assert float(kl0) == 0.0
    # ... and then nothing of the teacher reaches the gradient
    tn = torch.full_like(t, math.nan).to(DEV)
    sdn = s.to(DEV).requires_grad_(True)
    kd_token_loss(sdn, tn, labels.to(DEV), kd_alpha=0.8, kd_loss_scale=0.0)[0].backward()
    assert torch.equal(sdn.grad, sd0.grad)


def test_non_contiguous_and_misaligned_student():
    from onebit_amd.kd import kd_token_loss
    s, t, labels = _make(2, 3, 1000, torch.float32, seed=9)
    base, _, _ = _token_case(s, t, labels, 0.8, 1.0, "contiguous")
    # a [S, B, V] buffer viewed as [B, S, V]
    sp = s.permute(1, 0, 2).contiguous().to(DEV).permute(1, 0, 2).requires_grad_(True)
    assert not sp.is_contiguous()
    kd_token_loss(sp, t.to(DEV), labels.to(DEV), kd_alpha=0.8, kd_loss_scale=1.0)[0].backward()
    assert torch.equal(sp.grad, base.grad)
    # contiguous rows whose base is 4 bytes past a 16-byte boundary take the element-wise loads
    flat = torch.empty(s.numel() + 1, device=DEV)
    flat[1:].copy_(s.reshape(-1).to(DEV))
    so = flat[1:].view(2, 3, 1000).requires_grad_(True)
    assert so.is_contiguous() and so.data_ptr() % 16 == 4
    kd_token_loss(so, t.to(DEV), labels.to(DEV), kd_alpha=0.8, kd_loss_scale=1.0)[0].backward()
    assert _rel(so.grad, base.grad) <= 1e-6


def test_upstream_gradient_is_applied_in_fp32_before_rounding():
    from onebit_amd.kd import kd_token_loss
    for dtype in (torch.float32, torch.float16):
        s, t, labels = _make(2, 5, 320, dtype, seed=10, scale=8.0)       # probabilities down to e^-40: many tiny gradients
        grads = []
        for k in (1.0, 1024.0):
            sd = s.to(DEV).requires_grad_(True)
            loss, _, _ = kd_token_loss(sd, t.to(DEV), labels.to(DEV), kd_alpha=0.8, kd_loss_scale=1.0)
            (k * loss).backward()
            grads.append(sd.grad)
        g1, g2 = grads[0].float(), grads[1].float()
        if dtype == torch.float32:
            # a power of two scales every fp32 product and sum exactly (but for underflow)
            assert torch.allclose(g2, 1024 * g1, rtol=2.0 ** -23, atol=1e-30)
        else:
            normal = g1.abs() >= 2.0 ** -14                 # both roundings relative: 2^-11 each
            assert ((g2 - 1024 * g1).abs() <= 2.0 ** -10 * 1.001 * g2.abs())[normal].all()      # / (1 - 2^-11): relative to g2
            # entries that round to zero in fp16 at 1x survive at 1024x: the factor is applied before the rounding
            assert int(((g1 == 0) & (g2 != 0)).sum()) > 0
            s64 = _kd_ref.to64(s)
            (1024 * _kd_ref.token_loss(s64, t.double(), labels, 0.8, 1.0)[0]).backward()
            assert _rel(grads[1], s64.grad) <= 2e-3


def test_two_runs_are_bit_equal():
    from onebit_amd.kd import kd_hidden_loss, kd_token_loss
    s, t, labels = _make(2, 3, 32000, torch.float32, seed=11)
    out = []
    for _ in range(2):
        sd = s.to(DEV).requires_grad_(True)
        loss, kl, ce = kd_token_loss(sd, t.to(DEV), labels.to(DEV), kd_alpha=0.8, kd_loss_scale=1.0)
        loss.backward()
        out.append((loss.detach().clone(), kl.clone(), ce.clone(), sd.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    g = torch.Generator().manual_seed(12)
    hs, ht = torch.randn(77, 4096, generator=g).half(), torch.randn(77, 4096, generator=g).half()
    out = []
    for _ in range(2):
        hd = hs.to(DEV).requires_grad_(True)
        d = kd_hidden_loss([hd], [ht.to(DEV)])
        d.backward()
        out.append((d.detach().clone(), hd.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*out))


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("T,H", [(1, 8), (10, 64), (77, 4096), (5, 5120), (9, 100), (3, 8200), (6, 99)])
def test_hidden_loss_vs_restatement(T, H, dtype, pairs):
    """(3, 8200): a row longer than the 512-thread kernel keeps in registers, walked in two chunks; (6, 99): a pitch that does
    not keep groups of four aligned (element-wise loads).  In fp16 the upstream gradient is T * H / 4, as a loss scale would be (fp32 runs unscaled): an
    element of the gradient is about coef * 2 / (3 T H) here, and fp16 holds it to 11 bits (the 2e-3 bar) only as a normal
    number, i.e. above 6.1e-5."""
    from onebit_amd.kd import kd_hidden_loss
    g = torch.Generator().manual_seed(T + H + pairs)
    ss = [(3.0 * torch.randn(T, H, generator=g)).to(dtype) for _ in range(pairs)]
    ts = [(s.float() + 2.0 * torch.randn(T, H, generator=g)).to(dtype) for s in ss]
    sd = [s.to(DEV).requires_grad_(True) for s in ss]
    loss = kd_hidden_loss(sd, [t.to(DEV) for t in ts])
    assert loss.dtype == torch.float32 and loss.shape == ()
    s64 = [_kd_ref.to64(s) for s in ss]
    ref = _kd_ref.hidden_loss(s64, [t.double() for t in ts])
    _check_loss(loss, ref, 2e-5 * abs(float(ref)), f"hidden {(T, H)} {dtype} x{pairs}")
    coef = 0.25 * T * H if dtype == torch.float16 else 1.0          # fp32 holds the unscaled gradient: coef = g / T as it is
    (coef * loss).backward()
    (coef * ref).backward()
    for a, b in zip(sd, s64):
        assert a.grad.dtype == dtype and _rel(a.grad, b.grad) <= GRAD_BAR[dtype]


def test_hidden_zero_teacher_row_and_3d_states():
    from onebit_amd.kd import kd_hidden_loss
    g = torch.Generator().manual_seed(13)
    s = torch.randn(1, 64, generator=g)
    d = kd_hidden_loss([s.to(DEV)], [torch.zeros(1, 64, device=DEV)])
    # t^ = 0: d = |s^|^2, which is 1 up to the fp32 rounding of the norm and of the 64 squares (not bit-exactly 1)
    assert abs(float(d) - 1.0) <= 2e-5
    # [B, S, H] states are rows of H; a zero teacher row among others agrees with the restatement
    s3, t3 = torch.randn(2, 5, 64, generator=g), torch.randn(2, 5, 64, generator=g)
    t3[1, 2] = 0.0
    sd = s3.to(DEV).requires_grad_(True)
    d = kd_hidden_loss((sd,), (t3.to(DEV),))
    s64 = _kd_ref.to64(s3)
    ref = _kd_ref.hidden_loss([s64], [t3.double()])
    _check_loss(d, ref, 2e-5 * abs(float(ref)), "hidden 3-D")
    d.backward()
    ref.backward()
    assert sd.grad.shape == s3.shape and _rel(sd.grad, s64.grad) <= 2e-4


def test_kdloss_end_to_end_through_bitlinear():
    """A tiny train-mode BitLinear produces the student logits; the gradients of KDLoss reach its three parameters and its
    input and match the restatement chained through the train-mode layer's own restatement (oracle/train_ref.py)."""
    from onebit_amd.kd import KDLoss
    from onebit_amd.train import BitLinear
    from oracle.train_ref import BitLinear as RefBitLinear
    B, S, K, V = 2, 6, 64, 200
    g = torch.Generator().manual_seed(14)
    params = {"weight": 0.3 * torch.randn(V, K, generator=g),
              "weight_scale": 0.1 * (0.5 + torch.rand(V, generator=g)),
              "input_factor": 0.1 * (0.5 + torch.rand(K, generator=g))}
    x = torch.randn(B, S, K, generator=g)
    tx = x + 0.5 * torch.randn(B, S, K, generator=g)
    t_logits = 2.0 * torch.randn(B, S, V, generator=g)
    labels = torch.randint(0, V, (B, S), generator=g)
    labels[1, 2] = -100
    m = BitLinear(K, V).to(DEV)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(params[n])
    xd = x.to(DEV).requires_grad_(True)
    logits = m(xd)
    crit = KDLoss(kd_alpha=0.8, kd_beta=1.0, kd_loss_scale=1.0)
    # hidden states: the layer's input and its output; n_layers = 1, so only the input pair enters the loss
    loss = crit(logits, t_logits.to(DEV), labels.to(DEV), (xd, logits), (tx.to(DEV), t_logits.to(DEV)))
    loss.backward()

    r = RefBitLinear(K, V, dtype=torch.float64)
    with torch.no_grad():
        for n, p in r.named_parameters():
            p.copy_(params[n].double())
    x64 = _kd_ref.to64(x)
    rlogits = r(x64)
    rloss = _kd_ref.kd_loss(rlogits, t_logits.double(), labels, (x64, rlogits), (tx.double(), t_logits.double()), None,
                            kd_alpha=0.8, kd_beta=1.0, kd_loss_scale=1.0)
    rloss.backward()
    assert _rel(logits, rlogits) <= 2e-5
    _check_loss(loss, rloss, _loss_bar(float(rloss), S, rlogits.detach().float(), t_logits), "end to end loss")
    assert _rel(xd.grad, x64.grad) <= 2e-4
    rp = dict(r.named_parameters())
    for n, p in m.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, n
        assert _rel(p.grad, rp[n].grad) <= 2e-4, n
