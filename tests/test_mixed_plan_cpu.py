"""The schedules of tests/_mixed_plan.py (what tests/test_gpu_mixed_reference.py feeds ``onebit_mixed_step``) and the teeth of its
driver, without a GPU: (1) the schedules' invariants -- distinct slots per step, every slot's positions contiguous from 0, all 16
recorded positions of the 4096-token prompt mapped once per variant, every route regime met; (2) the driver on a stand-in step -- the
tiny golden model b in fp32 on the CPU, each slot's token history kept, module-path arithmetic on the whole history -- passes
``_parity_log.check`` against both goldens, and three planted faults (output rows shifted by one, two slots swapped, ``start`` off
by one) each trip the bar."""
import os

import numpy as np
import pytest
import torch

import _mixed_plan as P


def _z(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def _check_schedule(steps, n_slots, max_len, max_rows=None, all_mapped=True):
    """Distinct slots per step; per slot the positions run on from 0 (a slot may restart at 0: the next rider); 1 <= k <= rows;
    one expectation per output row."""
    length = {}
    for si, st in enumerate(steps):
        slots = [it[0] for it in st.items]
        assert len(slots) == len(set(slots)) and 1 <= len(slots) <= n_slots, si
        assert all(0 <= s < n_slots for s in slots), si
        for slot, start, toks, k in st.items:
            assert start == length.get(slot, 0) or start == 0, (si, slot, start, length.get(slot, 0))
            assert 1 <= k <= len(toks) and start + len(toks) <= max_len, (si, slot)
            length[slot] = start + len(toks)
        assert len(st.expect) == sum(it[3] for it in st.items), si
        if all_mapped:
            assert all(e is not None for e in st.expect), si
        if max_rows is not None:
            assert P.rows_of(st) <= max_rows, (si, P.rows_of(st))
    return length


def _mapped(steps, array):
    return [e[1] for st in steps for e in st.expect if e is not None and e[0] == array]


def test_classify_thresholds():
    got = {T: P.classify(T) for T in (1, 2, 64, 65, 128, 129, 191, 192, 320, 321, 4120)}
    R = P.REGIMES
    assert got == {1: R[0], 2: R[0], 64: R[0], 65: R[1], 128: R[1], 129: R[2], 191: R[2], 192: R[3], 320: R[3], 321: R[4], 4120: R[4]}
    assert len(set(R)) == 5


def test_long_schedules_cover_the_recorded_positions(golden_dir):
    z = _z(golden_dir, "model_wide_c")
    pos = [int(p) for p in z["long_pos"]]
    a = P.long_schedule(z, "A", slot=0)
    assert [len(st.items[0][2]) for st in a] == [93, 1076, 748, 190, 470, 166, 548, 12, 786] + [1] * 7
    assert [st.items[0][1] + len(st.items[0][2]) - 1 for st in a] == pos                # every item ends on a recorded position
    assert _check_schedule(a, 6, 4096) == {0: 4096}
    assert _mapped(a, "long_logits") == [(i,) for i in range(16)]
    assert sum(it[3] for st in a for it in st.items) == 16
    b = P.long_schedule(z, "B", slot=4)
    assert [(st.items[0][1], len(st.items[0][2])) for st in b] == [(0, 2107), (2107, 1982), (4089, 7)]
    assert b[2].items[0][3] == 7 and all(e is not None for e in b[2].expect)              # the tail: one chunk, lm_head on all 7 rows
    assert _check_schedule(b, 6, 4096, all_mapped=False) == {4: 4096}
    assert sorted(_mapped(b, "long_logits")) == [(i,) for i in range(16)]                 # each of the 16 exactly once
    # an unmapped output row of B is a row BETWEEN recorded positions of a long chunk, nothing else; the mapped ones sit at their position
    for st in b:
        slot, start, toks, k = st.items[0]
        first = start + len(toks) - k
        for j, e in enumerate(st.expect):
            assert (e is not None) == (first + j in pos)
            if e is not None:
                assert pos[e[1][0]] == first + j
    ids = z["long_ids"][0]
    for sched in (a, b):
        assert [t for st in sched for t in st.items[0][2]] == [int(t) for t in ids]      # the whole prompt, in order


def test_riders_make_every_regime_and_use_twelve_sequences(golden_dir):
    z = _z(golden_dir, "model_wide_c")
    base = P.long_schedule(z, "A", slot=0)
    steps = P.with_riders(base, z, [1, 2, 3])
    _check_schedule(steps, 6, 4096, max_rows=1100)
    assert [st.items[:1] for st in steps[:len(base)]] == [st.items for st in base]       # the long prompt's items unchanged, first in their steps
    assert _mapped(steps, "long_logits") == [(i,) for i in range(16)]
    assert sum(it[3] for st in steps for it in st.items) == sum(len(st.expect) for st in steps)
    # every rider that starts also finishes: prefill row + its three decode rows, in order, in one slot
    per_seq = {}
    for st in steps:
        for it, e in zip(st.items, st.expect):                                            # (k = 1 everywhere: one expectation per item)
            if e[0] == "batch_logits":
                per_seq.setdefault(e[1][0], []).append((e[1][1], it[0], it[1], len(it[2])))
    assert len(per_seq) >= 12 and sorted(per_seq) == list(range(len(per_seq)))
    for b, seq in per_seq.items():
        assert [(ph, start, n) for ph, _, start, n in seq] == [(0, 0, 6), (1, 6, 1), (2, 7, 1), (3, 8, 1)], b
        assert len({slot for _, slot, _, _ in seq}) == 1
        assert seq[0][1] in (1, 2, 3)
    toks = z["batch_greedy_f16"]
    for st in steps:
        for it, e in zip(st.items, st.expect):
            if e[0] == "batch_logits":
                b, ph = e[1]
                assert it[2] == ([int(t) for t in z["batch_ids"][b]] if ph == 0 else [int(toks[b, ph - 1])])
    # every route regime is met by a step that carries a recorded position of the long prompt, and thresholds from both sides
    regimes = {P.classify(P.rows_of(st)) for st in steps if any(e[0] == "long_logits" for e in st.expect)}
    assert regimes == set(P.REGIMES)
    T = [P.rows_of(st) for st in steps]
    assert T[:9] == [99, 1083, 756, 193, 478, 174, 556, 15, 794]
    assert P.classify(190) != P.classify(T[3]) and P.classify(93) == P.classify(T[0])
    # from step 1 to the end of the long prompt every step is mixed: decode rows next to at least one segment, or (the tail) a segment
    # next to the long prompt's own decode row
    for st in steps[1:len(base)]:
        n = [len(it[2]) for it in st.items]
        assert 1 in n and (max(n) > 1 or len(n) == 4)
    assert any(all(len(it[2]) == 1 for it in st.items) for st in steps)                   # and decode-only steps (no segment) occur


def test_short_and_batch_schedules(golden_dir):
    for name in ("model_tiny_a", "model_tiny_b", "model_tiny_bias", "model_wide_c", "model_wide_d", "model_wide_e"):
        z = _z(golden_dir, name)
        S, nd = z["input_ids"].shape[1], z["decode_logits_f16"].shape[1]
        assert np.array_equal(z["greedy_f16"], z["greedy_f32"])                           # teacher forcing is valid against both goldens
        for chunks in (None, [3, S - 3]):
            st = P.short_schedule(z, 1, chunks)
            assert _check_schedule(st, 2, S + nd) == {1: S + nd}
            assert _mapped(st, "prefill_logits") == [(0, p) for p in range(S)] and _mapped(st, "decode_logits") == [(0, i) for i in range(nd)]
        if "batch_ids" in z.files:
            assert np.array_equal(z["batch_greedy_f16"], z["batch_greedy_f32"])
            B, n = z["batch_ids"].shape[0], z["batch_logits_f16"].shape[1]
            st = P.batch_schedule(z, list(range(B)))
            _check_schedule(st, B, 6 + n - 1)
            assert sorted(_mapped(st, "batch_logits")) == [(b, i) for b in range(B) for i in range(n)]
            assert [P.rows_of(s) for s in st] == [6 * B] + [B] * (n - 1)


# ---- the driver on a stand-in step ------------------------------------------------------------------------------------------------------

class _StandIn:
    """What MixedStep.launch promises, in fp32 on the CPU: every slot's tokens by position; an item writes its tokens at ``start ...``
    (a gap reads as token 0, what follows the item is forgotten); the logits of its last ``k`` rows by the module path's arithmetic
    (y = LayerNorm((W . (h * x)) * g) + bias per projection, RMSNorm, rotary embedding, causal softmax attention, SwiGLU) on the slot's
    whole history."""

    def __init__(self, z):
        from oracle.oracle import np_int8_to_fp
        from onebit_amd.llama import OneBitLlamaConfig, rope_tables
        self.cfg = OneBitLlamaConfig(**{k[4:]: int(z[k]) for k in z.files if k.startswith("cfg_")})
        self.sd = {}
        for k in z.files:
            if k.startswith("sd_"):
                a = z[k]
                self.sd[k[3:]] = torch.from_numpy(np_int8_to_fp(a, np.float32)) if a.dtype == np.int8 else torch.from_numpy(a).float()
        self.cos, self.sin = rope_tables(self.cfg.head_dim, self.cfg.max_position_embeddings, self.cfg.rope_theta, "cpu", torch.float32)
        self.hist = {}

    def _lin(self, name, x):
        sd = self.sd
        u = ((x * sd[name + ".input_factor"]) @ sd[name + ".weight"].T) * sd[name + ".weight_scale"]
        y = torch.nn.functional.layer_norm(u, (u.shape[-1],), eps=1e-5)
        return y + sd[name + ".bias"] if name + ".bias" in sd else y

    def _rms(self, name, x):
        return self.sd[name + ".weight"] * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.cfg.rms_norm_eps))

    def forward(self, tokens):
        from onebit_amd.llama import _rotate_half
        cfg = self.cfg
        S, H, Hkv, D = len(tokens), cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        h = self.sd["model.embed_tokens.weight"][torch.tensor(tokens)]
        c, s = self.cos[:S][None], self.sin[:S][None]
        for l in range(cfg.num_hidden_layers):
            p = f"model.layers.{l}."
            x = self._rms(p + "input_layernorm", h)
            q = self._lin(p + "self_attn.q_proj", x).view(S, H, D).transpose(0, 1)
            k = self._lin(p + "self_attn.k_proj", x).view(S, Hkv, D).transpose(0, 1)
            v = self._lin(p + "self_attn.v_proj", x).view(S, Hkv, D).transpose(0, 1)
            q, k = q * c + _rotate_half(q) * s, k * c + _rotate_half(k) * s
            k, v = k.repeat_interleave(H // Hkv, dim=0), v.repeat_interleave(H // Hkv, dim=0)
            w = q @ k.transpose(1, 2) / D ** 0.5 + torch.triu(torch.full((S, S), float("-inf")), diagonal=1)
            o = (torch.softmax(w, -1) @ v).transpose(0, 1).reshape(S, H * D)
            h = h + self._lin(p + "self_attn.o_proj", o)
            x = self._rms(p + "post_attention_layernorm", h)
            act = torch.nn.functional.silu(self._lin(p + "mlp.gate_proj", x)) * self._lin(p + "mlp.up_proj", x)
            h = h + self._lin(p + "mlp.down_proj", act)
        return self._rms("model.norm", h) @ self.sd["lm_head.weight"].T

    def launch(self, items):
        out = []
        for slot, start, toks, k in items:
            hist = (self.hist.get(slot, []) + [0] * start)[:start] + [int(t) for t in toks]
            self.hist[slot] = hist
            out.append(self.forward(hist)[len(hist) - k:])
        lg = torch.cat(out).numpy()
        return lg, lg.argmax(axis=1)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    z = _z(golden_dir, "model_tiny_b")
    # the 8-token prompt in chunks 3 + 5 (k = 3 and 5), then the 4 teacher-forced single-token items, in slot 0; the same prompt whole
    # (k = 8) and its decode steps in slot 2 two steps later, so that a step holds two items at DIFFERENT positions (a swap shows)
    steps = P.merge(P.short_schedule(z, 0, [3, 5]), P.short_schedule(z, 2), offset=2)
    _check_schedule(steps, 3, 12)
    return z, steps


def test_stand_in_passes_the_reference_bar(tiny):
    z, steps = tiny
    rec = P.drive(_StandIn(z).launch, steps, z, "model_tiny_b", "stand-in (fp32, CPU)")
    assert sorted(i for r in rec if r["array"] == "prefill_logits" for i in r["index"]) == sorted([(0, p) for p in range(8)] * 2)
    assert sorted(i for r in rec if r["array"] == "decode_logits" for i in r["index"]) == sorted([(0, i) for i in range(4)] * 2)
    for r in rec:
        assert r["e16"] <= r["bar"] and r["e32"] <= r["bar"]


def _faulty(z, fault):
    real = _StandIn(z)
    calls = [0]

    def launch(items):
        calls[0] += 1
        if fault == "rows shifted by one":
            lg, nxt = real.launch(items)
            return np.roll(lg, 1, axis=0), np.roll(nxt, 1)
        if fault == "two slots swapped" and len(items) == 2 and calls[0] == 4:              # one step hands two items each other's slot
            (s0, a0, t0, k0), (s1, a1, t1, k1) = items
            items = [(s1, a0, t0, k0), (s0, a1, t1, k1)]
        if fault == "start off by one":
            items = [(s, a + 1, t, k) for s, a, t, k in items]
        return real.launch(items)
    return launch


@pytest.mark.parametrize("fault", ["rows shifted by one", "two slots swapped", "start off by one"])
def test_planted_faults_trip_the_bar(tiny, fault):
    z, steps = tiny
    with pytest.raises(AssertionError, match=r"step \d+: T = \d+ \(skinny<=64\), output row \d+ of item \(slot \d, start \d+, \d tokens, k \d\).*error.*bar"):
        P.drive(_faulty(z, fault), steps, z, "model_tiny_b", "stand-in with a planted fault")
