"""Host restatement of the sampling contract (include/onebit.h, onebit_sample_params_t) for the tests: numpy only.

``sample_row`` returns the token the contract defines for one fp16 logits row, the kept set, and whether the row is
ambiguous: the device computes the Gumbel noise and the softmax masses in fp32 / fixed point, this module in float64, so a
row whose two best perturbed scores, or whose top-p boundary mass, lie within 1e-5 (relative) of each other may
legitimately come out either way.  Everything else -- the temperature division, the top-k threshold, the Philox stream -- is
exact and must agree bit for bit.
"""
import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF
AMBIG = 1e-5


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Random123): ctr = four uint32 arrays (broadcast), key = (k0, k1) -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in ctr]
    c = np.broadcast_arrays(*c)
    c = [x.copy() for x in c]
    k0, k1 = np.uint64(key[0] & _MASK), np.uint64(key[1] & _MASK)
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & np.uint64(_MASK), p1 & np.uint64(_MASK),
             ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & np.uint64(_MASK), p0 & np.uint64(_MASK)]
        k0 = (k0 + np.uint64(_W0)) & np.uint64(_MASK)
        k1 = (k1 + np.uint64(_W1)) & np.uint64(_MASK)
    return [x.astype(np.uint32) for x in c]


def gumbel(V, seed_lo, seed_hi, stream, n):
    """g_i for i < V at sequence index n (float64)."""
    i = np.arange(V, dtype=np.uint64)
    words = philox4x32_10((np.uint64(n & _MASK), np.uint64(stream & _MASK), i >> np.uint64(2), np.uint64(0)), (seed_lo, seed_hi))
    r = np.choose((i & np.uint64(3)).astype(np.int64), words).astype(np.uint64)
    u = ((r >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def greedy(logits16):
    h = np.asarray(logits16, dtype=np.float16).astype(np.float32)
    ok = h > -np.inf                                   # NaN compares false
    if not ok.any():
        return 0
    m = h[ok].max()
    return int(np.flatnonzero(ok & (h == m))[0])


def scores(logits16, temperature):
    h = np.asarray(logits16, dtype=np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        s = (h / np.float32(temperature)).astype(np.float32)
    s[np.isnan(s)] = -np.inf
    return s


def is_sampled(do_sample, temperature):
    t = np.float32(temperature)
    return bool(do_sample) and bool(t > 0) and bool(np.isfinite(t))


def kept_set(s, top_k, top_p, alternatives=False):
    """Kept mask after top-k then top-p on fp32 scores s (no +inf, not all -inf), and the distance of the top-p boundary
    masses to top_p (inf when top-p is off).  With ``alternatives``: also the kept masks a boundary mass within AMBIG of top_p
    could give instead (the last kept score group dropped, or the next one kept)."""
    V = s.shape[0]
    keep = np.ones(V, dtype=bool)
    if 0 < top_k < V:
        kth = np.sort(s)[::-1][top_k - 1]
        keep = s >= kth
    dist, alts = np.inf, []
    tp = np.float32(top_p)
    if not np.isnan(tp) and tp < 1:
        sk = s[keep].astype(np.float64)
        smax = sk.max()
        e = np.exp(sk - smax)
        p = e / e.sum()
        vals = np.unique(sk)[::-1]                          # distinct kept scores, descending
        mass = np.array([p[sk == v].sum() for v in vals])
        above = np.concatenate([[0.0], np.cumsum(mass)])    # above[j]: mass strictly above vals[j]; above[-1] = 1
        stay = above[:-1] < float(tp)
        stay[0] = True                                      # the maximum always stays
        j = int(np.flatnonzero(stay).max())                 # last kept group; above[j + 1] is the first mass >= top_p
        cand = [abs(above[j + 1] - float(tp))] + ([abs(above[j] - float(tp))] if j > 0 else [])
        dist = float(min(cand))
        base = keep.copy()
        keep = base & (s.astype(np.float64) >= vals[j])
        if j > 0 and abs(above[j] - float(tp)) < AMBIG:
            alts.append(base & (s.astype(np.float64) >= vals[j - 1]))
        if j + 1 < len(vals) and abs(above[j + 1] - float(tp)) < AMBIG:
            alts.append(base & (s.astype(np.float64) >= vals[j + 1]))
    return (keep, dist, alts) if alternatives else (keep, dist)


def sample_row(logits16, do_sample=1, temperature=1.0, top_k=0, top_p=1.0, seed=0, stream=0, n=0):
    """(token, kept mask or None for a greedy / degenerate row, ambiguous)."""
    logits16 = np.asarray(logits16, dtype=np.float16)
    V = logits16.shape[0]
    if not is_sampled(do_sample, temperature):
        return greedy(logits16), None, False
    s = scores(logits16, temperature)
    if not (s > -np.inf).any():
        return 0, None, False
    if (s == np.inf).any():
        return int(np.flatnonzero(s == np.inf)[0]), None, False
    keep, dist, alts = kept_set(s, int(top_k), top_p, alternatives=True)
    g = gumbel(V, seed & _MASK, (seed >> 32) & _MASK, stream, n)
    sc = np.where(keep, s.astype(np.float64) + g, -np.inf)
    tok = int(np.argmax(sc))
    # a top-p boundary that could fall the other way matters only if it changes the token
    ambiguous = any(int(np.argmax(np.where(k, s.astype(np.float64) + g, -np.inf))) != tok for k in alts)
    if keep.sum() > 1:
        order = np.argsort(-sc, kind="stable")
        a, b = sc[order[0]], sc[order[1]]
        if np.isfinite(b):
            scale = max(1.0, abs(a), abs(b), abs(s[order[0]]), abs(g[order[0]]), abs(s[order[1]]), abs(g[order[1]]))
            ambiguous |= abs(a - b) <= AMBIG * scale
    return tok, keep, bool(ambiguous)


def warped_probs(logits16, temperature, top_k, top_p):
    """The distribution the draw samples from: softmax of s over the kept set (float64)."""
    s = scores(logits16, temperature)
    keep, _ = kept_set(s, int(top_k), top_p)
    z = np.where(keep, s.astype(np.float64), -np.inf)
    e = np.exp(z - z.max())
    return e / e.sum(), keep
