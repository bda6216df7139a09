"""Schedules that pin ``onebit_mixed_step`` to the reference's RECORDED logits, and the driver that runs them.

A schedule is a list of ``Step(items, expect)``: ``items`` are the ``(slot, start, tokens, k)`` tuples of ``MixedStep.launch``;
``expect`` has one entry per output row of the step, in the order ``launch`` returns them (items in the order given, each its last
``k`` rows): ``(golden array, index)`` -- the row must equal ``z[array + "_f16"][index]`` / ``z[array + "_f32"][index]`` -- or ``None``
for a row no golden covers (only the long chunks of ``long_schedule(z, "B")`` have such rows, see there).

Every token fed is the reference's own (prompt ids, ``greedy_f16`` / ``batch_greedy_f16``: teacher forcing; the fixtures' fp16 and
fp32 greedy tokens are equal, so both goldens hold for every row).  Plain Python + numpy: nothing here touches torch or a GPU, the
CPU suite runs the same driver on a stand-in step (tests/test_mixed_plan_cpu.py)."""
from collections import namedtuple

import numpy as np

import _parity_log

Step = namedtuple("Step", "items expect")

# the row-count thresholds of onebit_mixed.hip's routing at its default switches (the test sets none)
REGIMES = ("skinny<=64", "passes65-128", "passes+kslices129-191", "grouped|passes+kslices192-320", "grouped>320")


def classify(T):
    """The mixed step's route by row count T (onebit_mixed.hip): <= 64 one skinny launch per projection group; 65 .. 320 balanced
    passes of <= 64 rows, o_proj / down_proj as K-slices from 129 rows on; from 192 rows q|k|v and gate|up may take the grouped LDS-DMA
    GEMM, above 320 they always do (with or without a skinny tail; hidden-width projections K-sliced or, when their tiles alone
    fill the chip, one GEMM each).  For failure messages and the coverage assertions only."""
    if T <= 64:
        return REGIMES[0]
    if T <= 128:
        return REGIMES[1]
    if T < 192:
        return REGIMES[2]
    if T <= 320:
        return REGIMES[3]
    return REGIMES[4]


def rows_of(step):
    return sum(len(it[2]) for it in step.items)


def short_schedule(z, slot, chunks=None):
    """The fixture's short prompt (``input_ids``) in ``slot``: as chunks of the given lengths (default: one chunk), lm_head on every row
    (``k`` = the chunk's length) against ``prefill_logits``; then one single-token item per recorded decode step, fed
    ``greedy_f16[0, i]`` at position ``len + i``, against ``decode_logits[0, i]``."""
    ids = [int(t) for t in z["input_ids"][0]]
    chunks = [len(ids)] if chunks is None else list(chunks)
    assert sum(chunks) == len(ids) and min(chunks) >= 1
    steps, p = [], 0
    for n in chunks:
        steps.append(Step([(slot, p, ids[p:p + n], n)], [("prefill_logits", (0, p + j)) for j in range(n)]))
        p += n
    toks = z["greedy_f16"][0]
    for i in range(z["decode_logits_f16"].shape[1]):
        steps.append(Step([(slot, p + i, [int(toks[i])], 1)], [("decode_logits", (0, i))]))
    return steps


def batch_schedule(z, slots):
    """All batch sequences at once: ``batch_ids[b]`` as a 6-row segment in ``slots[b]`` (last row = ``batch_logits[b, 0]``), then the
    recorded decode steps as decode-only steps (no segment), fed ``batch_greedy_f16[b, i]``, against ``batch_logits[b, 1 + i]``."""
    bids, toks = z["batch_ids"], z["batch_greedy_f16"]
    B, S = bids.shape
    assert len(slots) == B and len(set(slots)) == B
    steps = [Step([(slots[b], 0, [int(t) for t in bids[b]], 1) for b in range(B)], [("batch_logits", (b, 0)) for b in range(B)])]
    for i in range(z["batch_logits_f16"].shape[1] - 1):
        steps.append(Step([(slots[b], S + i, [int(toks[b, i])], 1) for b in range(B)], [("batch_logits", (b, 1 + i)) for b in range(B)]))
    return steps


def long_schedule(z, variant, slot=0):
    """The 4096-token prompt (``long_ids``) whose logits the reference recorded at the 16 positions ``long_pos``.
    "A": cut after every recorded position -- each chunk's last row is a recorded one (k = 1); the positions that follow each other
         directly at the end of the prompt become single-token items: decode rows at a context of ~4090 keys.
    "B": cut after positions 2106 and 4088 only, and the remaining rows as ONE chunk with k = all of them: the tail positions go
         through the ragged flash attention instead of the split-KV decode attention.  So that all 16 positions are compared in this
         variant too, the two long chunks ask lm_head for every row from their first recorded position on (k = 2015 and 1513, the
         lm_head loop over more than 64 rows); the rows between recorded positions have no golden: ``None``."""
    ids = [int(t) for t in z["long_ids"][0]]
    pos = [int(p) for p in z["long_pos"]]
    assert pos == sorted(set(pos)) and pos[-1] == len(ids) - 1
    if variant == "A":
        steps, p0 = [], 0
        for i, p in enumerate(pos):
            steps.append(Step([(slot, p0, ids[p0:p + 1], 1)], [("long_logits", (i,))]))
            p0 = p + 1
        return steps
    if variant != "B":
        raise ValueError(variant)
    cuts = [2106, 4088, pos[-1]]
    assert all(c in pos for c in cuts)
    steps, p0 = [], 0
    for c in cuts:
        inside = [i for i, p in enumerate(pos) if p0 <= p <= c]
        first = pos[inside[0]]
        at = {pos[i]: i for i in inside}
        expect = [("long_logits", (at[p],)) if p in at else None for p in range(first, c + 1)]
        steps.append(Step([(slot, p0, ids[p0:c + 1], c + 1 - first)], expect))
        p0 = c + 1
    assert all(e is not None for e in steps[-1].expect) and len(steps[-1].expect) == len(steps[-1].items[0][2])   # the tail: k = its rows
    return steps


def with_riders(steps, z, rider_slots):
    """The batch sequences riding along: rider slot j takes its first sequence in step j; a sequence enters as a 6-row segment
    (``batch_logits[b, 0]``), decodes in the next steps fed ``batch_greedy_f16[b, i]`` at position 6 + i (``batch_logits[b, 1 + i]``),
    then the slot goes to the next sequence, which overwrites the cache rows from position 0.  The slots are one step out of phase,
    so from step 1 on every step carries decode rows AND a segment.  After the last of ``steps`` the sequences in flight finish in
    steps of their own (decode rows only); no new one starts there."""
    bids, toks = z["batch_ids"], z["batch_greedy_f16"]
    B, S = bids.shape
    nd = z["batch_logits_f16"].shape[1] - 1
    used = {it[0] for st in steps for it in st.items}
    assert not used & set(rider_slots) and len(set(rider_slots)) == len(rider_slots)
    state = {s: None for s in rider_slots}               # slot -> (sequence, phase): phase 0 = enters, 1 .. nd = decode step phase - 1
    nxt, out, i = 0, [], 0
    while i < len(steps) or any(v is not None for v in state.values()):
        base = steps[i] if i < len(steps) else Step([], [])
        items, expect = list(base.items), list(base.expect)
        for j, s in enumerate(rider_slots):
            if state[s] is None and i < len(steps) and i >= j and nxt < B:
                state[s] = (nxt, 0)
                nxt += 1
            if state[s] is None:
                continue
            b, ph = state[s]
            if ph == 0:
                items.append((s, 0, [int(t) for t in bids[b]], 1))
            else:
                items.append((s, S + ph - 1, [int(toks[b, ph - 1])], 1))
            expect.append(("batch_logits", (b, ph)))
            state[s] = (b, ph + 1) if ph < nd else None
        out.append(Step(items, expect))
        i += 1
    return out


def merge(a, b, offset=0):
    """Two schedules on disjoint slots in the same steps, ``b`` starting ``offset`` steps after ``a``."""
    out = []
    for i in range(max(len(a), len(b) + offset)):
        items, expect = [], []
        for sched, j in ((a, i), (b, i - offset)):
            if 0 <= j < len(sched):
                items += sched[j].items
                expect += sched[j].expect
        out.append(Step(items, expect))
    return out


def bar_of(z, array):
    """The bar of a golden array: ``_parity_log.loose_tol`` of the WHOLE array (a compared slice keeps it)."""
    return _parity_log.loose_tol(z[array + "_f16"], z[array + "_f32"])


def _log_name(array, index):
    # (the names _parity_log.OBSERVED and the profile lines of the other routes use for the batch goldens)
    if array == "batch_logits":
        return "batch_prefill" if index[1] == 0 else "batch_decode"
    return array


def drive(launch, steps, z, fixture, route, before_step=None):
    """Run ``steps`` through ``launch(items) -> (logits [n_out, V], next_tokens [n_out])`` (numpy) and hold every mapped output row
    to the reference: per step and golden array ONE ``_parity_log.check`` (both goldens, the whole array's bar; the profile line names
    the step, its row count and its route), ``next_tokens`` = argmax of the returned row on EVERY output row, and = the reference's
    greedy token wherever the reference's top-2 margin exceeds 2 x the bar.  A failure names step, T, classify(T) and the item.
    ``before_step(step index, step)``, if given, runs before each launch (the GPU test re-poisons the cache rows the step must not read).
    Returns one record per compared group: dict(step, T, regime, array, index (list), e16, e32, bar)."""
    records = []
    for si, st in enumerate(steps):
        T, regime = rows_of(st), classify(rows_of(st))
        if before_step is not None:
            before_step(si, st)
        logits, nxt = launch(st.items)
        n_out = sum(it[3] for it in st.items)
        assert len(st.expect) == n_out and logits.shape[0] >= n_out and len(nxt) >= n_out, (si, n_out, logits.shape, len(nxt))
        logits = np.asarray(logits[:n_out], dtype=np.float32)
        nxt = np.asarray(nxt[:n_out]).astype(np.int64)
        item_of = [it for it in st.items for _ in range(it[3])]
        where = lambda r: "step %d: T = %d (%s), output row %d of item (slot %d, start %d, %d tokens, k %d)" % (
            (si, T, regime, r) + (item_of[r][0], item_of[r][1], len(item_of[r][2]), item_of[r][3]))
        assert np.isfinite(logits).all(), where(int(np.argwhere(~np.isfinite(logits).all(axis=1))[0, 0])) + ": logits not finite"
        am = logits.argmax(axis=1)
        bad = np.flatnonzero(nxt != am)
        assert bad.size == 0, where(int(bad[0])) + ": next token %d is not the argmax %d of its logits" % (nxt[bad[0]], am[bad[0]])
        groups = {}
        for r, e in enumerate(st.expect):
            if e is not None:
                groups.setdefault((e[0], _log_name(*e)), []).append(r)
        for (array, name), rows in groups.items():
            idx = [st.expect[r][1] for r in rows]
            ref16 = np.stack([z[array + "_f16"][i] for i in idx])
            ref32 = np.stack([z[array + "_f32"][i] for i in idx])
            bar = bar_of(z, array)
            got = logits[rows]
            try:
                e16, e32 = _parity_log.check(fixture, name, "%s step %d T=%d %s" % (route, si, T, regime), got, ref16, ref32, loose=bar)
            except AssertionError as exc:
                err = np.maximum(np.abs(got - ref16).max(axis=1), np.abs(got - ref32).max(axis=1))
                w = int(err.argmax())
                raise AssertionError("%s, %s%s: error %.5f, bar %.5f | %s" % (where(rows[w]), array, list(idx[w]), err[w], bar, exc)) from None
            srt = np.sort(ref16, axis=1)
            for r, ref, top2 in zip(rows, ref16, srt[:, -1] - srt[:, -2]):
                if top2 > 2.0 * bar:                                # the reference's own top-2 margin is not noise
                    assert nxt[r] == int(ref.argmax()), where(r) + ": token %d, the reference's %d (margin %.4f > 2 x bar)" % (nxt[r], int(ref.argmax()), top2)
            records.append(dict(step=si, T=T, regime=regime, array=array, index=idx, e16=e16, e32=e32, bar=bar))
    return records
