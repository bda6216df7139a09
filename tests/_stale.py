"""What one ``MixedStep`` step may depend on, and what it may not: the POISON PLAN of tests/test_gpu_mixed_stale_state.py, the
evaluation workload whose steps those tests run, and the bit-for-bit comparison they assert.  Plain Python + torch on whatever
device the tensors live on: tests/test_stale_cpu.py runs the same plan and the same comparison on a CPU stand-in.

A step reads its token rows, the model, the KV-cache rows ``0 .. start - 1`` of the slots it names, and the ARRIVAL TICKETS of the
split-KV decode attention (``ob_fdec.h``: zero between launches, the last split of a row puts its word back to zero).  Everything
else it touches it must write before it reads.  So these may hold anything before a launch:

  * the workspace AFTER the tickets.  The tickets are the first ``align256(n_slots * n_heads * 4)`` bytes (``ob_fdec_launch``: tickets
    first, their place depends on the slot count and the head count only); behind them lie the attention's ``{max, sum}`` words and
    partial outputs and every ``[rows, *]`` activation of the step, at offsets that depend on the step's OWN row count
    (``ob_mixed_carve``, restated in ``carve`` below) -- a smaller step after a larger one finds the larger one's bytes there.
  * ``logits`` and ``_part_val`` (floating point outputs / scratch of lm_head).
  * KV-cache rows: from ``start`` to the end of the slot for every slot the step names, every row of every other slot.
  * the integer buffers the step reads as indices or writes as outputs -- ``_part_idx``, ``next_tokens``, the staging rows beyond the
    step's own entries.  They are only ever filled with the IN-RANGE value 1: a read-before-write there must show as a wrong
    number, never become an address outside an allocation.

``PATTERNS`` are byte fills, so one fill serves fp16, fp32 and int alike:

    0x7b   fp16 61280 (finite)     fp32 ~1.3e36 (finite)
    0x7e   fp16 NaN                fp32 ~8.4e37 (finite)
    0xff   fp16 NaN                fp32 NaN

The finite pattern matters most: ``fmaxf`` and compares swallow NaN, and the one wrong result on record was finite."""
from collections import namedtuple

import torch

PATTERNS = (0x7b, 0x7e, 0xff)
CLASSES = ("workspace", "caches", "outputs")
MAX_SPLITS = 64           # OB_MIXED_MAX_SPLITS: the attention scratch is laid out for that many splits
MAX_OUT = 64              # OB_MIXED_MAX_OUT: rows per lm_head launch (the size of ``xh``)

Piece = namedtuple("Piece", "name off nbytes")
Dims = namedtuple("Dims", "hidden intermediate n_heads n_kv_heads head_dim")
Plan = namedtuple("Plan", "ws_lo ws_hi cache_from")


def align256(b):
    return (b + 255) & ~255


def ticket_bytes(n_slots, n_heads):
    return align256(n_slots * n_heads * 4)


def dims_of(cfg):
    return Dims(cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim)


def carve(dims, rows, n_slots):
    """``ob_mixed_carve(m, rows, n_slots, ...)`` restated: ``([Piece(name, offset, bytes)], total bytes)``, offsets from the 256-byte
    aligned workspace base, every piece rounded up to 256 bytes.  The attention scratch comes first and is laid out for ``n_slots``
    single-token rows whatever the step holds; it is listed as its two halves, ``tickets`` and ``attn_partials``."""
    H, I = dims.hidden, dims.intermediate
    NQ, NK = dims.n_heads * dims.head_dim, dims.n_kv_heads * dims.head_dim
    rh = n_slots * dims.n_heads
    tick = align256(rh * 4)
    scratch = align256(rh * MAX_SPLITS * 128 * 4) + align256(rh * MAX_SPLITS * 2 * 4) + tick
    pieces, off = [Piece("tickets", 0, tick), Piece("attn_partials", tick, scratch - tick)], align256(scratch)

    def take(name, nbytes):
        nonlocal off
        pieces.append(Piece(name, off, align256(nbytes)))
        off += align256(nbytes)
    T = rows
    for name in ("hA", "hB", "x", "xs0", "xs1", "xs2"):
        take(name, T * H * 2)
    take("uq", T * NQ * 2), take("uk", T * NK * 2), take("uv", T * NK * 2)
    take("q", T * NQ * 2), take("attn", T * NQ * 2), take("uo", T * H * 2)
    take("ug", T * I * 2), take("uu", T * I * 2), take("act", T * I * 2)
    take("ud", T * H * 2), take("xh", MAX_OUT * H * 2)
    take("gemm_ws", T * max(H, I, NQ) * 2)
    for i in range(4):
        take("z%d" % i, T * H * 4)
    return pieces, off


def plan(n_slots, n_heads, ws_bytes, items):
    """The poison plan of a step: the workspace bytes ``[ws_lo, ws_hi)`` (from the aligned base; everything after the tickets) and, per
    cache slot, the first row that may be poisoned -- ``start`` for a slot the step names (the rows before it are the request's
    past and stay), 0 for every other slot."""
    cache_from = {s: 0 for s in range(n_slots)}
    for it in items:
        slot, start = int(it[0]), int(it[1])
        assert 0 <= slot < n_slots and start >= 0 and cache_from[slot] == 0, "a repeated slot"
        cache_from[slot] = start
    tick = ticket_bytes(n_slots, n_heads)
    assert ws_bytes > tick
    return Plan(tick, int(ws_bytes), cache_from)


def _fill_bytes(t, byte):
    t.view(torch.uint8).fill_(byte)


def poison(step, caches, pl, byte, classes=CLASSES, ws_ranges=None):
    """Fill what ``pl`` allows on ``step`` (a ``MixedStep``, or a stand-in with its attributes) and its ``caches`` with ``byte``.
    ``classes``: which of workspace / caches / outputs.  ``ws_ranges``: ``[(lo, hi)]`` byte ranges of the workspace to fill instead of
    all of it (one carve piece at a time); they are clipped to the plan."""
    assert 0 <= byte <= 255 and set(classes) <= set(CLASSES)
    if "workspace" in classes:
        ws = step._ws[step._ws_off:]
        assert pl.ws_hi <= ws.numel()
        for lo, hi in ([(pl.ws_lo, pl.ws_hi)] if ws_ranges is None else ws_ranges):
            lo, hi = max(lo, pl.ws_lo), min(hi, pl.ws_hi)
            if lo < hi:
                ws[lo:hi].fill_(byte)
    if "caches" in classes:
        for kc, vc in caches:
            for slot, first in pl.cache_from.items():
                if first < kc.shape[2]:
                    _fill_bytes(kc[slot, :, first:], byte)
                    _fill_bytes(vc[slot, :, first:], byte)
    if "outputs" in classes:
        if step.logits is not None:
            _fill_bytes(step.logits, byte)
        _fill_bytes(step._part_val, byte)
        # index-typed buffers: the in-range value 1 only (token 1, slot 1, position 1, output row 1)
        step._part_idx.fill_(1)
        step.next_tokens.fill_(1)
        for t in list(step._h_stage) + list(step._d_stage):
            t.fill_(1)                       # (launch rewrites its own entries: what stays is the tail beyond the step's rows)


# ------------------------------------------------------------------------------------------------------------ comparison --
def out_rows(items):
    """[(item index, slot, row inside the segment)] per output row, in the order ``launch`` returns them."""
    rows = []
    for i, it in enumerate(items):
        n, k = len(it[2]), (int(it[3]) if len(it) > 3 else 1)
        rows += [(i, int(it[0]), r) for r in range(n - k, n)]
    return rows


def moved(a_logits, a_next, b_logits, b_next, items):
    """Output rows whose bits differ between two runs of one step: ``[(item, slot, row in segment, logits that differ, token a, token b)]``.
    Bits, not values: a NaN equals nothing, not even the same NaN."""
    rows = out_rows(items)
    n = len(rows)
    assert a_logits.shape[0] >= n and b_logits.shape[0] >= n and a_next.shape[0] >= n and b_next.shape[0] >= n
    al, bl = a_logits[:n].contiguous(), b_logits[:n].contiguous()
    assert al.dtype == bl.dtype == torch.float16
    nan = (torch.isnan(al) | torch.isnan(bl)).sum(dim=1)
    diff = ((al.view(torch.int16) != bl.view(torch.int16)).sum(dim=1) + nan).cpu().tolist()
    ta, tb = a_next[:n].cpu().tolist(), b_next[:n].cpu().tolist()
    return [(i, slot, r, d, x, y) for (i, slot, r), d, x, y in zip(rows, diff, ta, tb) if d or x != y]


def assert_same(a_logits, a_next, b_logits, b_next, items, what=""):
    """``torch.equal`` on the logits of every output row and on the tokens; a failure names the segments and rows that moved."""
    n = len(out_rows(items))
    if torch.equal(a_logits[:n], b_logits[:n]) and torch.equal(a_next[:n], b_next[:n]):
        return
    mv = moved(a_logits, a_next, b_logits, b_next, items)
    segs = sorted({m[0] for m in mv})
    worst = float((a_logits[:n].float() - b_logits[:n].float()).abs().nan_to_num(nan=float("inf")).max())
    raise AssertionError("%s: %d of %d output rows moved, largest |delta logit| %g; segments %s (rows of segment: %s); first rows "
                         "(item, slot, row in segment, logits that differ, token a, token b): %s" % (
                             what, len(mv), n, worst, segs, [len(items[i][2]) for i in segs], mv[:12]))


# ------------------------------------------------------------------------------------------------------------- workload --
EVAL_VOCAB, EVAL_BATCH, EVAL_MAX_LENGTH = 2048, 16, 400
# The row counts of the steps.  VERDICT.md names the steps of the failing test "5384 / 2620 / 88 rows": that is the 34 requests sorted and
# cut into chunks of 16 one by one.  ``loglikelihood_tokens`` first groups requests with identical tokens (request 32 repeats request
# 3), so what it launches is 33 items in steps of 5300 / 2459 / 1 rows.  Both sets are tested.
ROWS_ONE_BY_ONE = (5384, 2620, 88)
ROWS_GROUPED = (5300, 2459, 1)


def eval_model_config():
    from onebit_amd.llama import OneBitLlamaConfig
    return OneBitLlamaConfig(vocab_size=EVAL_VOCAB, hidden_size=1024, intermediate_size=2816, num_hidden_layers=3, num_attention_heads=8,
                             num_key_value_heads=4, max_position_embeddings=512)


def eval_requests():
    """The 34 requests of ``test_gpu_evaluate.py::test_loglikelihood_tokens_ragged_equals_padded_at_width``, built as that test builds them."""
    g = torch.Generator().manual_seed(1)
    reqs = []
    for i in range(32):
        n, c = int(torch.randint(44, 391, (1,), generator=g)), int(torch.randint(1, 9, (1,), generator=g))
        t = torch.randint(0, EVAL_VOCAB, (n,), generator=g).tolist()
        reqs.append((t[:-c], t[-c:]))
    reqs.append((reqs[3][0], reqs[3][1]))
    reqs.append(([5], [7]))
    return reqs


def eval_steps(reqs, grouped, batch_size=EVAL_BATCH, max_length=EVAL_MAX_LENGTH):
    """The requests as mixed steps: sorted by falling length (ties by tokens), cut into chunks of ``batch_size``, every request the item
    ``(its index in the chunk, 0, (context + continuation)[-(max_length + 1):][:-1], len(continuation))``.  ``grouped``: requests
    with the same tokens are one item, as ``loglikelihood_tokens`` launches them; else every request is an item of its own."""
    keyed = {}
    for i, (ctx, cont) in enumerate(reqs):
        toks = tuple(ctx) + tuple(cont)
        keyed.setdefault((-len(toks), toks) if grouped else (-len(toks), toks, i), (ctx, cont))
    order = sorted(keyed)
    steps = []
    for c0 in range(0, len(order), batch_size):
        items = []
        for key in order[c0:c0 + batch_size]:
            ctx, cont = keyed[key]
            items.append((len(items), 0, (list(ctx) + list(cont))[-(max_length + 1):][:-1], len(cont)))
        steps.append(items)
    return steps


def rows_of(items):
    return sum(len(it[2]) for it in items)


def mid_steps(T, vocab=EVAL_VOCAB, seed=0):
    """A priming step and a ``T``-row step for the routes the evaluation steps do not take: slots 0 .. 2 decode at 40, 170 and 300
    cached tokens (two attention splits of 256), slot 3 continues a 20-token prompt, slots 4 and 5 start one; slots 6 and 7 idle.
    -> (priming items, step items); run the priming step first, poison afterwards."""
    assert T >= 12
    g = torch.Generator().manual_seed(1000 + seed + T)
    tok = lambda n: torch.randint(0, vocab, (n,), generator=g).tolist()
    ctx = (40, 170, 300, 20)
    prime = [(s, 0, tok(n), 1) for s, n in enumerate(ctx)]
    a, b = (T - 3) // 2, (T - 3) // 3
    c = T - 3 - a - b
    step = [(s, ctx[s], tok(1), 1) for s in range(3)] + [(3, ctx[3], tok(a), 1), (4, 0, tok(b), min(2, b)), (5, 0, tok(c), 1)]
    assert rows_of(step) == T
    return prime, step
