"""The train-mode causal attention (onebit_amd/train_model.py: flash_attention_train -> onebit_attention_train_forward / _backward,
csrc/ob_flash_train.h): o, lse, dq, dk and dv against eager attention evaluated in float64 on the CPU (tests/_train_model_ref.py).

Every bar is ``_train_ref.MARGIN x`` the distance to that truth of the SAME eager restatement evaluated in float16 on the CPU, per
tensor, for max |a - b| / rms(b) and for the relative L2.  No number comes from the kernels.  One exception, with its reasoning:
at S = 1 dq and dk are zero in exact arithmetic (dS = P (dP - delta) with P = 1 and delta = P dP), so they have no scale of their
own.  The kernels recompute P = exp2(s c - lse log2e) from an lse that went through fp32 once (|1 - P| <= a few 2^-24 max(1, |s| c),
|s| c < 32 here) and form dP as an fp32 sum of D products, so |dP - delta| <= 2 D 2^-24 sum_d |dO_d v_d| with room to spare, and the
gradient is that times |k| (or |q|) / sqrt(D), plus one fp16 subnormal step.

Shapes: the smallest that reach each branch -- S around the 64-row block edges of both axes (a lone diagonal block, ragged tails,
several blocks), both head dims, MHA and two GQA ratios, one and two sequences.  Measured values and bars are written to
profiles/train_attention_parity.txt (or under OB_PROFILES_DIR) when OB_WRITE_PROFILES=1."""
import math
import os

import pytest
import torch

import _train_model_ref as M
import _train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TENSORS = ("o", "lse", "dq", "dk", "dv")

S_VALUES = (1, 15, 63, 64, 65, 127, 128, 129, 200, 321)
HEADS = ((2, 2), (4, 2), (4, 1))
# every S with both head dims; heads and batch cycle so that every listed value of every axis appears with small and large S
CASES = []
for _i, _S in enumerate(S_VALUES):
    for _j, _D in enumerate((64, 128)):
        _n = 2 * _i + _j
        CASES.append((_S, _D) + HEADS[_n % 3] + (1 + (_n // 3) % 2,))
# + the block-edge sizes once more with the other GQA ratios and batch sizes
for _i, _S in enumerate(S_VALUES):
    _j = (_i + 1) % 2
    _n = 2 * _i + _j
    CASES.append((_S, (64, 128)[_j]) + HEADS[(_n + 1) % 3] + (2 - (_n // 3) % 2,))
CASE_IDS = ["S%d-D%d-H%d-Hkv%d-B%d" % c for c in CASES]
assert {c[0] for c in CASES} == set(S_VALUES) and {c[1] for c in CASES} == {64, 128}
assert {c[2:4] for c in CASES} == set(HEADS) and {c[4] for c in CASES} == {1, 2} and len(set(CASES)) == len(CASES) == 30


def _hip(q, k, v):
    from onebit_amd.train_model import flash_attention_train
    return flash_attention_train(q, k, v, return_lse=True)


def _log(case_id, m, bar):
    if os.environ.get("OB_WRITE_PROFILES") != "1":
        return
    out_dir = os.environ.get("OB_PROFILES_DIR") or os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "train_attention_parity.txt"), "a") as f:
        for k, v in m.items():
            b = bar[k]
            f.write(f"{case_id:<28s} {k[0]:<4s} {k[1]:<5s} measured {v:.3e}  bar {b:.3e}  ratio {v / b if b > 0 else (0.0 if v == 0 else float('inf')):.3f}\n")


_TRUTH = {}


def _refs(case_id, case):
    """(float64 truth, float16-on-CPU restatement) of a case, once per process"""
    if case_id not in _TRUTH:
        _TRUTH[case_id] = (M.run_attention(case, torch.float64, lse_fn=M.ref_lse), M.run_attention(case, torch.float16, lse_fn=M.ref_lse))
    return _TRUTH[case_id]


def _zero_bar(case, name):
    """S = 1: the bound of the module docstring for dq (name "dq") / dk, per element maximum"""
    q, k, v, d_o = (case[n] for n in ("q", "k", "v", "d_o"))
    D, rep = q.shape[-1], q.shape[2] // k.shape[2]
    prod = (d_o * v.repeat_interleave(rep, dim=2)).abs().sum(-1)                  # [B, 1, H]
    slack = 2 * D * 2.0 ** -24 * float(prod.max())
    other = float((k if name == "dq" else q).abs().max())
    return (rep if name == "dk" else 1) * slack * other / math.sqrt(D) + 2.0 ** -24


def _check(case_id, case, got):
    truth, own = _refs(case_id, case)
    m, bar = {}, {}
    for n in TENSORS:
        assert got[n].shape == truth[n].shape and bool(torch.isfinite(got[n]).all()), n
        if float(truth[n].abs().max()) <= 1e-12:
            assert case["q"].shape[1] == 1 and n in ("dq", "dk"), (n, "zero in float64")
            m[(n, "abs")], bar[(n, "abs")] = float(got[n].abs().max()), _zero_bar(case, n)
            continue
        for name, metric in (("peak", R.peak), ("l2", R.l2)):
            m[(n, name)], bar[(n, name)] = metric(got[n], truth[n]), R.MARGIN * metric(own[n], truth[n])
    _log(case_id, m, bar)
    for k in m:
        print(case_id, k, "measured %.3e  bar %.3e" % (m[k], bar[k]))
    bad = {k: (m[k], bar[k]) for k in m if not m[k] <= bar[k]}
    assert not bad, bad


@pytest.mark.parametrize("shape", CASES, ids=CASE_IDS)
def test_parity_and_determinism(shape):
    S, D, H, Hkv, B = shape
    cid = "S%d-D%d-H%d-Hkv%d-B%d" % shape
    case = M.attention_case(B, S, H, Hkv, D, seed=1000 + CASES.index(shape))
    got = M.run_attention(case, torch.float16, fn=_hip, device=DEV)
    _check(cid, case, got)
    again = M.run_attention(case, torch.float16, fn=_hip, device=DEV)        # forward and backward twice: identical bits
    for n in TENSORS:
        assert torch.equal(got[n], again[n]), n


@pytest.mark.parametrize("D", [64, 128])
def test_scores_that_span_more_than_the_deferral_threshold(D):
    """three keys far above the rest (tests/_train_model_ref.py: "spread"): an early one (the running maximum jumps in the first
    block), one in the second block that exceeds it by ~4 log2 units (kept: P > 1 under the old maximum), a late one ~13 log2 units
    above that (the maximum moves again, the sums are rescaled).  lse and every gradient must come out the same."""
    S = 200
    case = M.attention_case(2, S, 4, 2, D, seed=77, kind="spread")
    sc = torch.einsum("bshd,bthd->bhst", case["q"], case["k"].repeat_interleave(2, dim=2)) / math.sqrt(D) * math.log2(math.e)
    row = sc[0, 0, S - 1]
    assert float(row.max() - row.median()) > 16.0 and int(row.argmax()) == S - 3          # > OB_FL_DEFER_THR = 8, twice over
    assert 2.0 < float(row[70] - row[1]) < 8.0 and float(row[S - 3] - row[70]) > 8.0
    _check("spread-D%d" % D, case, M.run_attention(case, torch.float16, fn=_hip, device=DEV))


def test_one_query_row_of_d_o_reaches_no_later_key():
    B, S, H, Hkv, D, r = 2, 200, 4, 2, 64, 77
    case = M.attention_case(B, S, H, Hkv, D, seed=5)
    d_o = torch.zeros_like(case["d_o"])
    d_o[:, r] = case["d_o"][:, r]
    case["d_o"] = d_o
    got = M.run_attention(case, torch.float16, fn=_hip, device=DEV)
    for n in ("dk", "dv"):
        assert bool((got[n][:, r + 1:] == 0).all()), (n, "a key after the only query with a gradient")
        assert float(got[n][:, :r + 1].abs().max()) > 0
    assert bool((got["dq"][:, :r] == 0).all()) and bool((got["dq"][:, r + 1:] == 0).all())
    _check("one-row", case, got)


GUARD = 4096
SENTINEL = 0xFF                                  # 0xFFFF / 0xFFFFFFFF: NaN in fp16 and fp32


def test_c_abi_writes_stay_inside_and_read_nothing_outside():
    """every tensor of both calls carved out of one arena of NaN bytes, >= 4 KiB of them around each: no guard byte changes, every
    output element is written with a finite value (so nothing outside the inputs was read into a result), and the bits are the
    module path's."""
    from onebit_amd import _lib
    from onebit_amd.bitnet import _stream_ptr
    lib = _lib.load()
    B, S, H, Hkv, D = 2, 129, 4, 2, 64
    case = M.attention_case(B, S, H, Hkv, D, seed=9)
    nws = lib.onebit_attention_train_workspace_bytes(B, S, H, Hkv, D)
    nq, nk = B * S * H * D * 2, B * S * Hkv * D * 2
    spec = [("q", nq), ("k", nk), ("v", nk), ("d_o", nq), ("o", nq), ("lse", B * H * S * 4), ("dq", nq), ("dk", nk), ("dv", nk), ("ws", nws)]
    off, spans = GUARD, {}
    for name, nbytes in spec:
        off = (off + 511) // 512 * 512 + (16 if name == "ws" else 0)
        spans[name] = (off, nbytes)
        off += nbytes + GUARD
    total = off
    arena = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
    base = arena.data_ptr()
    assert base % 512 == 0
    ptr = {n: base + o for n, (o, _) in spans.items()}
    for n in ("q", "k", "v", "d_o"):
        o, nbytes = spans[n]
        arena[o:o + nbytes] = case[n].to(torch.float16).contiguous().view(torch.uint8).flatten().to(DEV)
    before = arena.cpu()
    dev = torch.device(DEV)
    with torch.cuda.device(dev):
        s = _stream_ptr(dev)
        _lib.check(lib.onebit_attention_train_forward(ptr["q"], ptr["k"], ptr["v"], ptr["o"], ptr["lse"], B, S, H, Hkv, D, s),
                   "onebit_attention_train_forward")
        _lib.check(lib.onebit_attention_train_backward(ptr["q"], ptr["k"], ptr["v"], ptr["o"], ptr["lse"], ptr["d_o"], ptr["dq"], ptr["dk"],
                                                       ptr["dv"], ptr["ws"], nws, B, S, H, Hkv, D, s), "onebit_attention_train_backward")
    torch.cuda.synchronize()
    host = arena.cpu()
    keep = torch.ones(total, dtype=torch.bool)                  # guards and inputs: unchanged
    for n in ("o", "lse", "dq", "dk", "dv", "ws"):
        o, nbytes = spans[n]
        keep[o:o + nbytes] = False
    touched = torch.nonzero(keep & (host != before)).flatten()
    assert touched.numel() == 0, ("bytes written outside the outputs", touched[:8].tolist(), spans)

    def carve(name, dt, shape):
        o, nbytes = spans[name]
        return host[o:o + nbytes].clone().view(dt).view(shape)
    out = {"o": carve("o", torch.float16, (B, S, H, D)), "lse": carve("lse", torch.float32, (B, H, S)),
           "dq": carve("dq", torch.float16, (B, S, H, D)), "dk": carve("dk", torch.float16, (B, S, Hkv, D)),
           "dv": carve("dv", torch.float16, (B, S, Hkv, D))}
    ref = M.run_attention(case, torch.float16, fn=_hip, device=DEV)
    for n, t in out.items():
        assert bool(torch.isfinite(t).all()), (n, "sentinel or non-finite elements", int((~torch.isfinite(t)).sum()))
        assert torch.equal(t.double(), ref[n]), (n, "differs from the module path")


def test_forward_and_backward_allocate_nothing_of_size_s_squared():
    from onebit_amd.train_model import flash_attention_train
    B, H, S, D = 1, 4, 2048, 64
    g = torch.Generator(device=DEV).manual_seed(3)
    q, k, v = (torch.randn(B, S, H, D, device=DEV, dtype=torch.float16, generator=g).requires_grad_(True) for _ in range(3))
    d_o = torch.randn(B, S, H, D, device=DEV, dtype=torch.float16, generator=g)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    o = flash_attention_train(q, k, v)
    o.backward(d_o)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - base
    print("peak rise %.2f MiB, one fp16 probability tensor %.0f MiB" % (rise / 2 ** 20, B * H * S * S * 2 / 2 ** 20))
    assert rise < B * H * S * S * 2
    assert all(bool(torch.isfinite(t.grad).all()) for t in (q, k, v))
