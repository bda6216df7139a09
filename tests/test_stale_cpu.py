"""The poison plan and the comparison of tests/_stale.py on a CPU stand-in of ``MixedStep``: the plan leaves the arrival tickets and
every valid cache row alone and covers everything else; a stand-in step that reads ONE poisoned word of a class (workspace, cache
tail, logits, ``part_val``, an index buffer) fails the comparison the GPU tests assert; the helper's steps are the ones
``loglikelihood_tokens`` launches."""
import pytest
import torch

import _stale as S

DIMS = S.Dims(hidden=128, intermediate=352, n_heads=4, n_kv_heads=2, head_dim=32)
N_SLOTS, MAX_LEN, VOCAB = 6, 48, 64
SENTINEL = 0x55


class StandIn:
    """The buffers of a ``MixedStep`` as CPU tensors, carved by the restated formulas, and a "step" whose outputs are a fixed function of
    its tokens and of the cache rows before ``start``.  ``fault``: read one word the step has not written."""

    def __init__(self, max_rows, fault=None):
        self.n_slots, self.fault = N_SLOTS, fault
        self._rows = max_rows
        _, total = S.carve(DIMS, max_rows, N_SLOTS)
        self._ws_off = 256
        self._ws = torch.zeros(total + 256 + self._ws_off, dtype=torch.uint8)
        self.logits = torch.zeros(max_rows, VOCAB, dtype=torch.float16)
        nparts = -(-VOCAB // 128) * 64
        self._part_val = torch.zeros(nparts, dtype=torch.float32)
        self._part_idx = torch.zeros(nparts, dtype=torch.int32)
        self.next_tokens = torch.zeros(max_rows + N_SLOTS, dtype=torch.int32)
        self._h_stage = [torch.zeros(4 * max_rows + N_SLOTS, dtype=torch.int32) for _ in range(2)]
        self._d_stage = [torch.zeros(4 * max_rows + N_SLOTS, dtype=torch.int32) for _ in range(2)]
        shape = (N_SLOTS, DIMS.n_kv_heads, MAX_LEN, DIMS.head_dim)
        self.caches = [(torch.zeros(shape, dtype=torch.float16), torch.zeros(shape, dtype=torch.float16)) for _ in range(2)]

    def launch(self, items):
        T = S.rows_of(items)
        pieces = {p.name: p for p in S.carve(DIMS, T, N_SLOTS)[0]}
        ws = self._ws[self._ws_off:]
        kc = self.caches[0][0]
        st = self._h_stage[0]
        st[:T] = torch.tensor([t for it in items for t in it[2]], dtype=torch.int32)           # its own entries of the staging row
        o = 0
        for slot, start, toks, k in items:
            n = len(toks)
            past = kc[slot, :, :start].float().sum()                                            # valid rows: the step may read them
            for r in range(n - k, n):
                row = torch.arange(VOCAB, dtype=torch.float32) * 0.01 + float(sum(toks[:r + 1]) % 97) + past
                if self.fault == "workspace" and o == 0:
                    row = row + ws[pieces["uo"].off:pieces["uo"].off + 2].view(torch.float16).float()
                if self.fault == "partials" and o == 0:
                    row = row + ws[pieces["attn_partials"].off + 4:pieces["attn_partials"].off + 8].view(torch.float32)
                if self.fault == "cache" and o == 0:
                    row = row + kc[slot, 0, start + n, 0].float() if start + n < MAX_LEN else row
                if self.fault == "other slot" and o == 0:
                    row = row + kc[N_SLOTS - 1, 1, 0, 3].float()
                if self.fault == "logits" and o == 1:
                    row = row + self.logits[o].float()                                          # accumulates into what was there
                self.logits[o] = row.half()
                self.next_tokens[o] = int(self.logits[o].float().nan_to_num(nan=-1.0).argmax())
                if self.fault == "part_val" and o == 2:
                    self.next_tokens[o] = 3 if float(self._part_val[5]) != 0.0 else self.next_tokens[o]
                if self.fault == "index" and o == 0:
                    self.next_tokens[o] = self.next_tokens[o] + st[T + 2]                         # the staging row beyond its entries
                o += 1
        return self.next_tokens[:o]


ITEMS = [(2, 5, [3, 9, 4, 1], 2), (0, 0, [7, 7, 8], 3), (4, 11, [6], 1)]


def _valid(step, byte):
    """What the plan must leave alone, marked: the tickets and the cache rows before each item's start."""
    step._ws[step._ws_off:step._ws_off + S.ticket_bytes(N_SLOTS, DIMS.n_heads)] = byte
    for kc, vc in step.caches:
        for slot, start, _, _ in ITEMS:
            kc[slot, :, :start] = 0.25
            vc[slot, :, :start] = 0.25


def test_carve_is_contiguous_and_tickets_come_first():
    for rows in (1, 48, 95, 543):
        pieces, total = S.carve(DIMS, rows, N_SLOTS)
        assert pieces[0] == S.Piece("tickets", 0, S.ticket_bytes(N_SLOTS, DIMS.n_heads))
        off = 0
        for p in pieces:
            assert p.off == off and p.nbytes % 256 == 0 and p.nbytes > 0, p
            off += p.nbytes
        assert off == total
        assert [p.name for p in pieces[2:8]] == ["hA", "hB", "x", "xs0", "xs1", "xs2"] and pieces[-1].name == "z3"
        # the tickets do not move with the row count; every activation piece does
        assert pieces[1].nbytes == S.carve(DIMS, 1, N_SLOTS)[0][1].nbytes
    a = {p.name: p.off for p in S.carve(DIMS, 95, N_SLOTS)[0]}
    b = {p.name: p.off for p in S.carve(DIMS, 543, N_SLOTS)[0]}
    assert a["hA"] == b["hA"] and all(a[n] < b[n] for n in a if n not in ("tickets", "attn_partials", "hA"))


@pytest.mark.parametrize("byte", S.PATTERNS)
def test_plan_spares_the_tickets_and_the_valid_rows_and_covers_the_rest(byte):
    st = StandIn(max_rows=16)
    _valid(st, SENTINEL)
    pl = S.plan(N_SLOTS, DIMS.n_heads, st._ws.numel() - st._ws_off, ITEMS)
    S.poison(st, st.caches, pl, byte)
    tick = S.ticket_bytes(N_SLOTS, DIMS.n_heads)
    ws = st._ws[st._ws_off:]
    assert bool((ws[:tick] == SENTINEL).all()) and bool((ws[tick:] == byte).all())
    assert bool((st._ws[:st._ws_off] == 0).all())                                   # nothing in front of the aligned base either
    used = {it[0]: it[1] for it in ITEMS}
    for kc, vc in st.caches:
        for c in (kc, vc):
            for slot in range(N_SLOTS):
                first = used.get(slot, 0)
                assert bool((c[slot, :, :first] == 0.25).all()), slot
                assert bool((c[slot, :, first:].contiguous().view(torch.uint8) == byte).all()), slot
    assert bool((st.logits.view(torch.uint8) == byte).all()) and bool((st._part_val.view(torch.uint8) == byte).all())
    for t in [st._part_idx, st.next_tokens] + st._h_stage + st._d_stage:             # index buffers: the in-range value only
        assert bool((t == 1).all())


def test_patterns_are_what_the_table_says():
    as16 = lambda b: float(torch.tensor([b, b], dtype=torch.uint8).view(torch.float16))
    as32 = lambda b: float(torch.tensor([b] * 4, dtype=torch.uint8).view(torch.float32))
    assert as16(0x7b) == 61280.0 and 1.2e36 < as32(0x7b) < 1.4e36
    assert as16(0x7e) != as16(0x7e) and 8.3e37 < as32(0x7e) < 8.5e37
    assert as16(0xff) != as16(0xff) and as32(0xff) != as32(0xff)


def _run(fault, byte, classes=S.CLASSES, ws_ranges=None):
    out = []
    for poisoned in (False, True):
        st = StandIn(max_rows=16, fault=fault)
        _valid(st, 0)
        if poisoned:
            pl = S.plan(N_SLOTS, DIMS.n_heads, st._ws.numel() - st._ws_off, ITEMS)
            S.poison(st, st.caches, pl, byte, classes, ws_ranges)
        nxt = st.launch(ITEMS)
        out += [st.logits, nxt]
    return out


@pytest.mark.parametrize("byte", S.PATTERNS)
def test_a_sound_step_passes_the_comparison(byte):
    S.assert_same(*_run(None, byte), ITEMS, "sound")


@pytest.mark.parametrize("byte", S.PATTERNS)
@pytest.mark.parametrize("fault,cls,row", [("workspace", "workspace", 0), ("partials", "workspace", 0), ("cache", "caches", 0),
                                           ("other slot", "caches", 0), ("logits", "outputs", 1), ("part_val", "outputs", 2),
                                           ("index", "outputs", 0)])
def test_one_poisoned_word_fails_the_comparison(fault, cls, row, byte):
    a = _run(fault, byte)
    with pytest.raises(AssertionError, match="output rows moved"):
        S.assert_same(*a, ITEMS, fault)
    mv = S.moved(*a, ITEMS)
    rows = S.out_rows(ITEMS)
    assert [m[:3] for m in mv] == [rows[row]]                                       # the report names the row that read it, and only that one
    # one class at a time names the class
    for c in S.CLASSES:
        b = _run(fault, byte, classes=(c,))
        assert bool(S.moved(*b, ITEMS)) == (c == cls), (fault, c)


def test_one_carve_piece_at_a_time_names_the_piece():
    pieces, _ = S.carve(DIMS, S.rows_of(ITEMS), N_SLOTS)
    hit = [p.name for p in pieces[1:] if S.moved(*_run("workspace", 0x7b, ("workspace",), [(p.off, p.off + p.nbytes)]), ITEMS)]
    assert hit == ["uo"]
    # the ticket range is clipped out of whatever is asked for
    st = StandIn(max_rows=16)
    pl = S.plan(N_SLOTS, DIMS.n_heads, st._ws.numel() - st._ws_off, ITEMS)
    S.poison(st, st.caches, pl, 0x7b, ("workspace",), [(0, 4096)])
    tick = S.ticket_bytes(N_SLOTS, DIMS.n_heads)
    assert bool((st._ws[st._ws_off:st._ws_off + tick] == 0).all()) and bool((st._ws[st._ws_off + tick:st._ws_off + 4096] == 0x7b).all())


def test_eval_steps_are_the_failing_tests_steps(monkeypatch):
    """34 requests; one by one in chunks of 16 they are the 5384 / 2620 / 88 rows VERDICT.md names; grouped -- what ``loglikelihood_tokens``
    launches, recorded here from the product itself through a stand-in scorer -- 5300 / 2459 / 1."""
    from onebit_amd import evaluate
    reqs = S.eval_requests()
    assert len(reqs) == 34 and reqs[32] == reqs[3] and reqs[33] == ([5], [7])
    one, grp = S.eval_steps(reqs, grouped=False), S.eval_steps(reqs, grouped=True)
    assert tuple(S.rows_of(s) for s in one) == S.ROWS_ONE_BY_ONE == (5384, 2620, 88)
    assert tuple(S.rows_of(s) for s in grp) == S.ROWS_GROUPED == (5300, 2459, 1)
    assert [len(s) for s in one] == [16, 16, 2] and [len(s) for s in grp] == [16, 16, 1]
    # the segments of the wrong result on record: 375, 364 and 354 rows, items 1, 2 and 4 of the first step
    assert [len(one[0][i][2]) for i in (1, 2, 4)] == [375, 364, 354] and [len(grp[0][i][2]) for i in (1, 2, 4)] == [375, 364, 354]
    # every segment of the first one-by-one step has three 128-query blocks: 16 x 8 heads x 2 block pairs = 256 workgroups
    assert all(-(-len(it[2]) // 128) == 3 for it in one[0])

    class Scorer:
        def __init__(self):
            self.launched, self.logits = [], None

        def launch(self, items):
            self.launched.append([(s, p, list(t), k) for s, p, t, k in items])
            self.logits = torch.zeros(sum(it[3] for it in items), S.EVAL_VOCAB, dtype=torch.float16)

    sc = Scorer()
    monkeypatch.setattr(evaluate, "_ragged_scorer", lambda *a, **k: sc)
    evaluate.loglikelihood_tokens(torch.nn.Linear(1, 1), reqs, S.EVAL_BATCH, S.EVAL_MAX_LENGTH, ragged=True)
    assert sc.launched == grp
