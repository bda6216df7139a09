"""Host restatement of the SVID initialiser (onebit_amd/svid.py, include/onebit.h ``onebit_svid_*``) for the tests: what
``sklearn.decomposition.NMF(n_components=1, init='random', random_state=0)`` computes on ``|A|`` -- for one component its
coordinate descent is alternating least squares -- in float64 numpy.

Pinned by ``tests/golden/svid.npz`` (recorded from sklearn's own ``NMF``, ``tests/golden/gen_goldens_svid.py``);
``tests/test_svid_cpu.py`` checks that this module reproduces the fixture's iteration counts exactly and its vectors to the
precision sklearn computed them in.  Only tests import it; the product never does.
"""
import numpy as np


def init(X, random_state=0):
    """sklearn's ``init='random'`` draws: ``(w0 [N], h0 [K])`` in X's dtype; H is drawn first."""
    N, K = X.shape
    avg = np.sqrt(X.mean())
    rng = np.random.RandomState(random_state)
    h = avg * rng.standard_normal(size=(1, K)).astype(X.dtype, copy=False)
    w = avg * rng.standard_normal(size=(N, 1)).astype(X.dtype, copy=False)
    return np.abs(w)[:, 0], np.abs(h)[0]


def _pg(v, grad):
    return np.where(v == 0, np.minimum(0.0, grad), grad)


def step(X, w, h):
    """one alternating iteration in float64: ``(w, h, violation)``"""
    hh, xh = h @ h, X @ h
    viol = np.abs(_pg(w, w * hh - xh)).sum()
    if hh != 0:
        w = np.maximum(xh / hh, 0.0)
    ww, xw = w @ w, X.T @ w
    viol += np.abs(_pg(h, h * ww - xw)).sum()
    if ww != 0:
        h = np.maximum(xw / ww, 0.0)
    return w, h, viol


def nmf_rank1(A, tol=1e-4, max_iter=200, n_iter=None, random_state=0, w0=None, h0=None):
    """``(w, h, n_iter, ratios)`` on ``X = |A|``: the draws in the dtype sklearn computes in (float32 for float32 input, float64
    after its promotion of anything else), the iterations in float64.  ``n_iter``: run exactly that many.  ``ratios[i]`` is
    violation / first violation after iteration i + 1."""
    X = np.abs(np.asarray(A))
    if X.dtype != np.float32:
        X = X.astype(np.float64)
    if w0 is None:
        w0, h0 = init(X, random_state)
    X = X.astype(np.float64)
    w, h = np.asarray(w0, dtype=np.float64), np.asarray(h0, dtype=np.float64)
    viol0, ratios, it = None, [], 0
    for it in range(1, (max_iter if n_iter is None else n_iter) + 1):
        w, h, viol = step(X, w, h)
        if it == 1:
            viol0 = viol
        ratios.append(viol / viol0 if viol0 != 0 else 0.0)
        if n_iter is None and (viol0 == 0 or viol / viol0 <= tol):
            break
    return w, h, it, ratios


def rel_residual(A, w, h):
    """``sqrt(sum (|a| - w_i h_j)^2 / sum a^2)`` in float64 (0 for the all-zero matrix)"""
    X = np.abs(np.asarray(A, dtype=np.float64))
    s1 = (X * X).sum()
    return float(np.sqrt(((X - np.outer(w, h)) ** 2).sum() / s1)) if s1 > 0 else 0.0


def max_rel(a, b):
    """largest element-wise gap relative to the largest element of ``b`` (0 when both are all zero)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max() if b.size else 0.0
    gap = np.abs(a - b).max() if b.size else 0.0
    return float(gap / scale) if scale > 0 else float(gap)


# ---- the model-level case: a seeded 2-layer teacher (hidden 256, inter 688, vocab 320), generated, never committed -----------
MODEL_SEED, MODEL_LAYERS, MODEL_HIDDEN, MODEL_INTER, MODEL_VOCAB, MODEL_HEADS = 8, 2, 256, 688, 320, 4
PROJS = (("self_attn.q_proj", "h", "h"), ("self_attn.k_proj", "h", "h"), ("self_attn.v_proj", "h", "h"), ("self_attn.o_proj", "h", "h"),
         ("mlp.gate_proj", "i", "h"), ("mlp.up_proj", "i", "h"), ("mlp.down_proj", "h", "i"))


def teacher_arrays():
    """the teacher's state dict as float32 numpy arrays in LLaMA's key order; no projection weight is exactly 0"""
    rng = np.random.RandomState(MODEL_SEED)
    dims = {"h": MODEL_HIDDEN, "i": MODEL_INTER}
    sd = {"model.embed_tokens.weight": (0.02 * rng.standard_normal((MODEL_VOCAB, MODEL_HIDDEN))).astype(np.float32)}
    for l in range(MODEL_LAYERS):
        for name, n, k in PROJS:
            a = rng.standard_normal((dims[n], dims[k])) * np.exp(0.5 * rng.standard_normal((dims[n], 1))) * np.exp(0.5 * rng.standard_normal((1, dims[k])))
            a = (0.02 * a).astype(np.float32)
            a[a == 0] = 1e-3
            sd[f"model.layers.{l}.{name}.weight"] = a
        sd[f"model.layers.{l}.input_layernorm.weight"] = (1.0 + 0.1 * rng.standard_normal(MODEL_HIDDEN)).astype(np.float32)
        sd[f"model.layers.{l}.post_attention_layernorm.weight"] = (1.0 + 0.1 * rng.standard_normal(MODEL_HIDDEN)).astype(np.float32)
    sd["model.norm.weight"] = (1.0 + 0.1 * rng.standard_normal(MODEL_HIDDEN)).astype(np.float32)
    sd["lm_head.weight"] = (0.02 * rng.standard_normal((MODEL_VOCAB, MODEL_HIDDEN))).astype(np.float32)
    return sd


def proj_keys():
    return [f"model.layers.{l}.{name}" for l in range(MODEL_LAYERS) for name, _, _ in PROJS]
