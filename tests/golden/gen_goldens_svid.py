"""Records tests/golden/svid.npz from sklearn's own NMF (needs scikit-learn; run by hand, never by the tests):

    python tests/golden/gen_goldens_svid.py

Every case calls ``sklearn.decomposition.NMF(n_components=1, init='random', random_state=0)`` -- the reference's three arguments
(``scripts/build_start_ckpt.py:21``) -- on ``|A|`` and records A, W, H, n_iter_, sklearn's own initial draws, the float64 top
singular triple of ``|A|``, and the violation ratios of the float64 restatement (tests/_svid_ref.py) at the stopping iteration
and the one before.  A case is kept only when both ratios are at least a factor 2 away from tol = 1e-4 (other seeds are tried
until one is), so that fp32 rounding cannot flip the iteration count.  ``fp32_gap`` is the largest relative gap (max element)
over the fp32 cases between sklearn's fp32 result and the float64 restatement at the same iteration count: the reference's own
rounding noise, which the GPU tests' tolerance is a multiple of.
"""
import os
import sys

import numpy as np
from sklearn.decomposition import NMF
from sklearn.decomposition._nmf import _initialize_nmf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _svid_ref  # noqa: E402

TOL = 1e-4


def make(name, seed):
    """the matrices by case name; every value from numpy.random.RandomState"""
    rng = np.random.RandomState(seed)
    base = lambda n, k: (0.02 * rng.standard_normal((n, k)) * np.exp(0.4 * rng.standard_normal((n, 1))) * np.exp(0.4 * rng.standard_normal((1, k))))
    if name == "n1_k8":
        return base(1, 8).astype(np.float32)
    if name == "zeros_37x72":                       # exact zeros, -0.0, an all-zero row
        a = base(37, 72).astype(np.float32)
        a[rng.rand(37, 72) < 0.05] = 0.0
        a[rng.rand(37, 72) < 0.03] = -0.0
        a[11, :] = 0.0
        return a
    if name == "outrow_48x64":                      # an outlier row
        a = base(48, 64).astype(np.float32)
        a[5, :] *= 15.0
        return a
    if name == "outcol_136x344":                    # an outlier column and an all-zero column
        a = base(136, 344).astype(np.float32)
        a[:, 77] *= 12.0
        a[:, 200] = 0.0
        return a
    if name == "tall_344x136":                      # more than one band step, an all-zero row, an outlier row and column
        a = base(344, 136).astype(np.float32)
        a[300, :] = 0.0
        a[17, :] *= 10.0
        a[:, 3] *= 20.0
        return a
    if name == "wide_24x2080":
        return base(24, 2080).astype(np.float32)
    if name == "half_40x136":
        return base(40, 136).astype(np.float16)
    if name == "f64_40x72":                         # float64 storage of fp32-representable values: sklearn computes in float64
        return base(40, 72).astype(np.float32).astype(np.float64)
    if name == "allzero_16x24":
        return np.zeros((16, 24), dtype=np.float32)
    raise KeyError(name)


CASES = ["n1_k8", "zeros_37x72", "outrow_48x64", "outcol_136x344", "tall_344x136", "wide_24x2080", "half_40x136", "f64_40x72", "allzero_16x24"]


def fit(a):
    x = np.abs(a)
    model = NMF(n_components=1, init="random", random_state=0)
    w = model.fit_transform(x)
    return w[:, 0], model.components_[0], int(model.n_iter_)


def margins_ok(a, n_iter):
    """(ok, ratio at the stop, ratio before it) of the float64 restatement, which must stop where sklearn stopped"""
    _, _, it, ratios = _svid_ref.nmf_rank1(a)
    if it != n_iter:
        return False, 0.0, 0.0
    last = ratios[-1]
    prev = ratios[-2] if len(ratios) > 1 else np.inf
    if it == 1:                                      # stops at once only when the first violation is 0 (ratio 0 / 0)
        return True, last, prev
    return (last <= TOL / 2 and prev >= 2 * TOL), last, prev


def main():
    out, fp32_gap = {}, 0.0
    for name in CASES:
        for seed in range(100, 200):
            a = make(name, seed)
            w, h, n_iter = fit(a)
            ok, last, prev = margins_ok(a, n_iter)
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed keeps the stopping rule a factor 2 from tol")
        x = np.abs(a) if a.dtype == np.float32 else np.abs(a).astype(np.float64)
        w0, h0 = _initialize_nmf(x, 1, init="random", random_state=0)
        wr, hr, _, _ = _svid_ref.nmf_rank1(a, n_iter=n_iter)
        gap = max(_svid_ref.max_rel(w, wr), _svid_ref.max_rel(h, hr))
        if a.dtype == np.float32:
            fp32_gap = max(fp32_gap, gap)
        u, s, vt = np.linalg.svd(np.abs(a).astype(np.float64), full_matrices=False)
        sign = 1.0 if u[:, 0].sum() >= 0 else -1.0
        out.update({f"{name}_A": a, f"{name}_W": w, f"{name}_H": h, f"{name}_n_iter": np.int64(n_iter), f"{name}_seed": np.int64(seed),
                    f"{name}_w0": w0[:, 0], f"{name}_h0": h0[0], f"{name}_mean": x.mean(), f"{name}_gap": np.float64(gap),
                    f"{name}_ratio_stop": np.float64(last), f"{name}_ratio_prev": np.float64(prev),
                    f"{name}_sv": np.float64(s[0]), f"{name}_su": sign * u[:, 0], f"{name}_svt": sign * vt[0]})
        print(f"{name:16s} seed {seed} dtype {a.dtype} n_iter {n_iter} ratio {prev:.3e} -> {last:.3e} gap {gap:.3e} W {w.dtype}")
    out["cases"] = np.array(CASES)
    out["fp32_gap"] = np.float64(fp32_gap)

    # the model-level case: the reference recipe on the seeded 2-layer teacher (weights regenerated by the test, not stored)
    sd = _svid_ref.teacher_arrays()
    keys, dtypes, model_gap = [], [], 0.0
    for k, v in sd.items():
        stem = k[:-len(".weight")]
        if stem in _svid_ref.proj_keys():
            assert (v == 0).sum() == 0
            w, h, n_iter = fit(v)
            ok, last, prev = margins_ok(v, n_iter)
            assert ok, (stem, n_iter, last, prev, "choose another MODEL_SEED in tests/_svid_ref.py")
            wr, hr, _, _ = _svid_ref.nmf_rank1(v, n_iter=n_iter)
            model_gap = max(model_gap, _svid_ref.max_rel(w, wr), _svid_ref.max_rel(h, hr))
            out.update({f"model/{stem}.weight_scale": w, f"model/{stem}.input_factor": h, f"model/{stem}.n_iter": np.int64(n_iter)})
            # torch.sign(A) * 0.01, torch.from_numpy(W / H): the dtypes of A and of sklearn's result for it
            keys += [k, stem + ".weight_scale", stem + ".input_factor"]
            dtypes += [str(v.dtype), str(w.dtype), str(h.dtype)]
            print(f"{stem:36s} n_iter {n_iter} ratio {prev:.3e} -> {last:.3e}")
        else:
            keys.append(k)
            dtypes.append(str(v.dtype))
    out["model_keys"], out["model_dtypes"], out["model_gap"] = np.array(keys), np.array(dtypes), np.float64(model_gap)
    print(f"fp32_gap {fp32_gap:.3e}  model_gap {model_gap:.3e}")
    path = os.path.join(HERE, "svid.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
