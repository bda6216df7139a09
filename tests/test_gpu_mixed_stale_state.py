"""``onebit_mixed_step`` must not depend on what its buffers held before the launch (tests/_stale.py states what it may read).

The model and the requests are those of ``test_gpu_evaluate.py::test_loglikelihood_tokens_ragged_equals_padded_at_width`` -- 1024 wide,
3 layers, 8 heads over 4 kv heads, 34 requests -- whose ragged route gave a wrong, finite, bit-reproducible result in two of three
whole-suite runs and never in a process of its own.  Its steps, both as VERDICT.md counts them (5384 / 2620 / 88 rows: the
requests one by one) and as ``loglikelihood_tokens`` launches them (5300 / 2459 / 1 rows: request 32 grouped with request 3):

  a. poisoned = clean, bit for bit: everything the poison plan allows (workspace behind the tickets, ``logits``, ``_part_val``, cache
     rows from ``start`` on and idle slots; index buffers with the in-range value 1) filled with 0x7b (finite in fp16 and fp32),
     0x7e and 0xff after construction.  The step has no atomics on data, so the bar is ``torch.equal``.  A failure reruns with one
     class and then one carve piece at a time and names class, piece, segments and rows.
  b. the product's sequence on ONE object built as ``_ragged_scorer`` builds it (``max_rows=64``: the workspace grows once, then is
     carved again at two smaller sizes) = every step on a fresh object; and in the opposite order.
  c. placement: caches as views 16 bytes into larger tensors, the workspace 0 / 256 / 3840 bytes into a poisoned one.
  d. lm_head on EVERY row of the 5384-row step against ``OneBitLlamaForCausalLM(cfg, torch.float32)`` on the padded batch, per segment,
     at the project's bar ``max(1.6 x gap + half an fp16 ulp, 2e-3 x scale)`` (tests/_parity_log.py), gap = the fp16 module path's
     distance from the fp32 one on the same rows.  error / gap per segment: profiles/mixed_stale_state.txt.
  e. (a) with 0x7b at 48, 95, 287 and 543 rows -- 3 decode rows at 40 / 170 / 300 cached tokens + prompt chunks, primed by a clean
     step -- for the skinny, balanced-pass and grouped routes.  The route is the one tests/_mixed_plan.py ``classify`` names from the
     library's default thresholds; it is not observed here (``OB_MIXED_SK_ROWS`` is latched inside the library on first use), and
     neither is what follows, which is read off ``ob_gemm3_ksplit_n`` for 256 CUs, not asserted.  K-slices: at these widths o_proj (K = 1024: four 256-column quads, one
     slice) is never K-sliced; down_proj (K = 2816) runs as TWO slices into ``z0`` / ``z1`` wherever its tiles alone leave a third of
     256 CUs idle, i.e. from 129 to 5376 rows -- the 287-, 543-, 2459-, 2620- and 5300-row steps here; the 5384-row step (43 row tiles) is
     the first that does not.  ``z2`` / ``z3`` (three and four slices, K >= 3072) are not reached by this model and are left to
     ``test_gpu_mixed.py::test_mixed_step_mid_size_routes``."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _mixed_plan as P
import _parity_log
import _stale as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_SLOTS, MAX_LEN = 16, 382                     # what loglikelihood_tokens gives _ragged_scorer for these requests


@pytest.fixture(scope="module")
def model():
    from onebit_amd.llama import build_synthetic_model
    return build_synthetic_model(S.eval_model_config(), seed=5, device=torch.device(DEV))


@pytest.fixture(scope="module")
def steps():
    reqs = S.eval_requests()
    one, grp = S.eval_steps(reqs, grouped=False), S.eval_steps(reqs, grouped=True)
    assert tuple(S.rows_of(s) for s in one) == (5384, 2620, 88) and tuple(S.rows_of(s) for s in grp) == (5300, 2459, 1)
    assert max(len(it[2]) for s in one for it in s) == MAX_LEN
    return {"one by one": one, "grouped": grp}


def _caches(cfg, n_slots, max_len, offset=0, fill=0):
    """Zeroed caches; ``offset``: each a contiguous view that many elements into a larger tensor filled with the byte ``fill``."""
    shape = (n_slots, cfg.num_key_value_heads, max_len, cfg.head_dim)
    n = int(np.prod(shape))

    def one():
        parent = torch.full((n + offset + 24,), 0, dtype=torch.float16, device=DEV)
        parent.view(torch.uint8).fill_(fill)
        t = parent[offset:offset + n].view(shape)
        assert t.is_contiguous() and t.data_ptr() == parent.data_ptr() + 2 * offset
        return t
    return [(one(), one()) for _ in range(cfg.num_hidden_layers)]


def _n_out(items):
    return sum(it[3] for it in items)


def _new(model, max_rows, n_slots=N_SLOTS, max_len=MAX_LEN, caches=None, n_out=0):
    """A MixedStep with room for ``max_rows`` rows and -- ``launch`` would otherwise drop ``logits`` for a fresh, zeroed tensor when a
    step has more output rows than slots -- for ``n_out`` rows of logits, so that nothing is allocated after the poison."""
    from onebit_amd.engine import MixedStep
    caches = _caches(model.config, n_slots, max_len) if caches is None else caches
    ms = MixedStep(model, caches, n_slots=n_slots, max_len=max_len, max_rows=max_rows, keep_logits=True)
    ms._ensure_logits(n_out)
    assert ms.logits.shape[0] >= max(n_out, n_slots)
    return ms, caches


def _buffers(ms):
    return [t.data_ptr() for t in [ms.logits, ms._ws, ms.next_tokens, ms._part_val, ms._part_idx] + list(ms._d_stage) + list(ms._h_stage)]


def _run(ms, items, fixed=True):
    """One step.  ``fixed``: the launch must keep every buffer it was given (a reallocation would swap poisoned bytes for zeros)."""
    before = _buffers(ms)
    nxt = ms.launch(items)
    torch.cuda.synchronize()
    n_out = _n_out(items)
    assert nxt.shape[0] == n_out
    assert not fixed or _buffers(ms) == before, "launch reallocated a buffer"
    return ms.logits[:n_out].clone(), nxt.clone()


def _greedy(lg, nxt):
    """Every token is a maximum of its row of logits (equal fp16 maxima: either index)."""
    return torch.equal(lg.gather(1, nxt.long().unsqueeze(1)).squeeze(1), lg.amax(dim=1))


def _plan(ms, items):
    return S.plan(ms.n_slots, ms.cfg.num_attention_heads, ms._ws.numel() - ms._ws_off, items)


@pytest.fixture(scope="module")
def clean(model, steps):
    """Every step once on an object left as constructed (zeros everywhere), ``max_rows`` = the step's rows: the values b and c also hold."""
    out = {}
    for name, sts in steps.items():
        for i, items in enumerate(sts):
            ms, _ = _new(model, S.rows_of(items), n_out=_n_out(items))
            out[name, i] = _run(ms, items)
            lg = out[name, i][0]
            assert bool(torch.isfinite(lg).all()) and _greedy(*out[name, i])
    return out


def _poisoned_run(model, items, byte, max_rows, classes=S.CLASSES, piece=None, n_slots=N_SLOTS, max_len=MAX_LEN, prime=None):
    ms, caches = _new(model, max_rows, n_slots, max_len, n_out=_n_out(items))
    if prime is not None:
        _run(ms, prime)
    ranges = None
    if piece is not None:
        ranges = [(piece.off, piece.off + piece.nbytes)]
    S.poison(ms, caches, _plan(ms, items), byte, classes, ranges)
    torch.cuda.synchronize()
    return _run(ms, items)


def _diagnose(model, items, byte, ref, max_rows, **kw):
    """After a failure: one class at a time, then (workspace) one carve piece at a time -> text for the assertion."""
    found = []
    for c in S.CLASSES:
        got = _poisoned_run(model, items, byte, max_rows, classes=(c,), **kw)
        mv = S.moved(*ref, *got, items)
        if not mv:
            continue
        found.append("class %s: %d rows, segments %s" % (c, len(mv), sorted({m[0] for m in mv})))
        if c == "workspace":
            for p in S.carve(S.dims_of(model.config), S.rows_of(items), kw.get("n_slots", N_SLOTS))[0][1:]:
                mvp = S.moved(*ref, *_poisoned_run(model, items, byte, max_rows, classes=(c,), piece=p, **kw), items)
                if mvp:
                    found.append("  piece %s [%d, %d): %d rows, segments %s" % (p.name, p.off, p.off + p.nbytes, len(mvp), sorted({m[0] for m in mvp})))
    return "; ".join(found) if found else "no single class reproduces it"


def test_restated_carve_is_the_librarys(model, steps):
    """The library exports only the TOTAL of its carve, and that is what pins ``_stale.carve`` for every row count below; two pieces swapped
    in order or size would keep the total (the piece-at-a-time diagnosis would then name the wrong piece).  Two offsets are pinned from
    what a step leaves behind on a zeroed workspace: the first activation (``hA``) starts where the attention scratch ends, and
    ``xh`` -- the final norm's rows, ``n_out`` of 64 written -- lies where the sizes of every piece before it put it."""
    from onebit_amd import _lib
    lib = _lib.load()
    dims = S.dims_of(model.config)
    for rows, ns in ((64, 16), (88, 16), (5384, 16), (543, 8), (1, 3)):
        ms, _ = _new(model, rows, n_slots=ns)
        assert ms._rows == max(rows, 64)
        nb = int(lib.onebit_mixed_workspace_bytes(ctypes.byref(ms._model), ms._rows, ns, ms.attn_chunk))
        assert S.carve(dims, ms._rows, ns)[1] == nb and ms._ws.numel() == nb + 256
    items = steps["one by one"][2]                                  # 87 rows + one decode row at position 0: one attention split, no partials
    T, n_out, row = S.rows_of(items), _n_out(items), 2 * dims.hidden
    ms, _ = _new(model, T, n_out=n_out)
    _run(ms, items)
    pc = {p.name: p for p in S.carve(dims, T, N_SLOTS)[0]}
    ws = ms._ws[ms._ws_off:]
    assert n_out < S.MAX_OUT and int(ws[:pc["hA"].off].max()) == 0 and int(ws[pc["hA"].off:pc["hA"].off + row].max()) > 0
    xh = pc["xh"]
    assert all(int(ws[xh.off + r * row:xh.off + (r + 1) * row].max()) > 0 for r in range(n_out))
    assert int(ws[xh.off + n_out * row:xh.off + xh.nbytes].max()) == 0


@pytest.mark.parametrize("byte", S.PATTERNS, ids=["0x7b", "0x7e", "0xff"])
@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("name", ["one by one", "grouped"])
def test_poisoned_equals_clean(model, steps, clean, name, i, byte):
    items = steps[name][i]
    T = S.rows_of(items)
    got = _poisoned_run(model, items, byte, T)
    try:
        S.assert_same(*clean[name, i], *got, items, "%s step %d (%d rows), everything poisoned with 0x%02x" % (name, i, T, byte))
    except AssertionError as e:
        raise AssertionError("%s | %s" % (e, _diagnose(model, items, byte, clean[name, i], T))) from None


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
@pytest.mark.parametrize("name", ["one by one", "grouped"])
def test_carry_over_between_steps_equals_fresh_objects(model, steps, clean, name, order):
    from onebit_amd.llama import KVCache
    kv = KVCache(model.config, N_SLOTS, MAX_LEN, torch.device(DEV), torch.float16)
    ms, _ = _new(model, 64, caches=kv.layers)
    assert ms._rows == 64
    bad = []
    for i in order:
        items = steps[name][i]
        got = _run(ms, items, fixed=False)                 # (growing is what this test is about)
        try:
            S.assert_same(*clean[name, i], *got, items, "%s step %d (%d rows) after steps %s on one object (capacity %d rows)" % (
                name, i, S.rows_of(items), [S.rows_of(steps[name][j]) for j in order[:order.index(i)]], ms._rows))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)
    assert ms._rows >= max(S.rows_of(s) for s in steps[name])


@pytest.mark.parametrize("name", ["one by one", "grouped"])
def test_placement_of_caches_and_workspace(model, steps, clean, name):
    items = steps[name][0]
    T = S.rows_of(items)
    caches = _caches(model.config, N_SLOTS, MAX_LEN, offset=8, fill=0x7b)
    assert all(c.data_ptr() % 32 == 16 for kc_vc in caches for c in kc_vc)
    ms, _ = _new(model, T, caches=caches, n_out=_n_out(items))
    total = ms._ws.numel() - 256
    tick = S.ticket_bytes(N_SLOTS, model.config.num_attention_heads)
    bad = []
    for off in (0, 256, 3840):
        parent = torch.full((total + 256 + 4096,), 0x7b, dtype=torch.uint8, device=DEV)
        base = (-parent.data_ptr()) % 256 + off
        parent[base:base + tick] = 0
        ms._ws, ms._ws_off = parent, base
        assert (ms._ws.data_ptr() + ms._ws_off) % 256 == 0 and ms._ws.numel() - ms._ws_off >= total
        S.poison(ms, caches, _plan(ms, items), 0x7b, ("caches", "outputs"))
        torch.cuda.synchronize()
        got = _run(ms, items)
        assert int(parent[base:base + tick].max()) == 0                               # the tickets are back at zero
        try:
            S.assert_same(*clean[name, 0], *got, items, "%s %d-row step, caches 16 bytes into their tensors, workspace at +%d" % (name, T, off))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


def test_every_row_of_the_5384_row_step_against_fp32(model, steps):
    """Per segment: the worst row of the mixed step's logits against the fp32 module path (and the fp16 one), its position, error / bar."""
    from onebit_amd.llama import OneBitLlamaForCausalLM
    cfg = model.config
    items = [(s, p, t, len(t)) for s, p, t, _ in steps["one by one"][0]]
    T = S.rows_of(items)
    assert T == 5384 and len(items) == 16
    ms, _ = _new(model, T, n_out=T)
    lg, nxt = _run(ms, items)
    assert lg.shape == (T, cfg.vocab_size) and bool(torch.isfinite(lg).all())
    assert _greedy(lg, nxt)
    m32 = OneBitLlamaForCausalLM(cfg, torch.float32)
    m32.load_state_dict({k: (v if v.dtype == torch.int8 else v.float()) for k, v in model.state_dict().items()})
    m32 = m32.to(torch.device(DEV)).eval()
    batch = torch.zeros(len(items), MAX_LEN, dtype=torch.long)
    for b, it in enumerate(items):
        batch[b, :len(it[2])] = torch.tensor(it[2])
    batch = batch.to(DEV)
    with torch.no_grad():
        l32, l16 = m32(batch), model(batch)
    l32 = (l32["logits"] if isinstance(l32, dict) else l32).float()
    l16 = (l16["logits"] if isinstance(l16, dict) else l16).float()
    lines, over, r0 = [], [], 0
    for b, it in enumerate(items):
        n = len(it[2])
        got, r32, r16 = lg[r0:r0 + n].float(), l32[b, :n], l16[b, :n]
        r0 += n
        gap = float((r16 - r32).abs().max())
        bar = _parity_log.loose_tol(r16.cpu().numpy(), r32.cpu().numpy())
        e32, e16 = (got - r32).abs().amax(dim=1), (got - r16).abs().amax(dim=1)
        w = int(torch.maximum(e32, e16).argmax())
        line = "segment %2d (%3d rows): worst row %3d  vs fp32 %.5f (%.2f x gap)  vs fp16 module path %.5f (%.2f x gap)  gap %.5f  bar %.5f  error / bar %.2f" % (
            b, n, w, float(e32[w]), float(e32[w]) / max(gap, 1e-12), float(e16[w]), float(e16[w]) / max(gap, 1e-12), gap, bar,
            max(float(e32[w]), float(e16[w])) / bar)
        lines.append(line)
        if float(e32.max()) > bar or float(e16.max()) > bar:
            over.append(line)
    print("\n".join(lines))
    if os.environ.get("OB_WRITE_PROFILES") == "1":
        os.makedirs(os.path.join(_parity_log.ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(_parity_log.ROOT, "profiles", "mixed_stale_state.txt"), "a") as f:
            f.write("5384-row step, lm_head on every row, 1024-wide 3-layer model: mixed step vs the fp32 / fp16 module path on the padded batch\n")
            f.write("\n".join(lines) + "\n")
    assert not over, "\n".join(over)


MID = {48: P.REGIMES[0], 95: P.REGIMES[1], 287: P.REGIMES[3], 543: P.REGIMES[4]}


@pytest.mark.parametrize("T", sorted(MID))
def test_poisoned_equals_clean_on_the_other_routes(model, T):
    assert P.classify(T) == MID[T]
    prime, items = S.mid_steps(T)
    kw = dict(n_slots=8, max_len=512, prime=prime)
    assert max(it[1] + len(it[2]) for it in prime + items) <= 512 and sum(len(it[2]) == 1 for it in items) == 3
    ms, _ = _new(model, 543, 8, 512, n_out=_n_out(items))
    _run(ms, prime)
    ref = _run(ms, items)
    assert bool(torch.isfinite(ref[0]).all())
    got = _poisoned_run(model, items, 0x7b, 543, **kw)
    try:
        S.assert_same(*ref, *got, items, "%d-row step (%s), everything poisoned with 0x7b after the priming step" % (T, MID[T]))
    except AssertionError as e:
        raise AssertionError("%s | %s" % (e, _diagnose(model, items, 0x7b, ref, 543, **kw))) from None

