"""Speculative decoding on the single-stream engine (prompt-lookup drafts), on the GPU:
  * ob_spec_commit_kernel            = tests/_spec_ref.py, exactly (every field of the record and of the next step's inputs)
  * onebit_attention_decode_rows_mq  = onebit_attention_decode_rows row by row, bit for bit; repeat launches identical; tickets zero
  * the verify pass                  teacher-forced against the reference's fp16 / fp32 logits (tests/_parity_log.loose_tol)
  * generate(..., speculative=)      the tokens of generate(...), greedy and sampled; golden / repeating / adversarial / oracle drafts;
                                     the end of the cache, the short-to-key-block hand-over, a growing split count
  * generate(..., speculative=None)  launches exactly the kernels of prime() + step() x (n - 1), the path of the parent commit
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from _spec_ref import commit_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEAR_TIE_USES = []            # (test, detail): every use of the near-tie rule is counted and printed


def _lib():
    from onebit_amd import _lib as L
    return L, L.load()


def _sp():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# ------------------------------------------------------------------------------------------------------ the commit kernel --
def _commit(lib, L, chosen, drafts, pos, remaining, history, max_len, nmax, nmin):
    from onebit_amd.engine import _SpecState
    dev = torch.device(DEV)
    k = len(drafts)
    ti = lambda v: torch.tensor(list(v), dtype=torch.int32, device=dev)
    hist = torch.full((max_len,), -7, dtype=torch.int32, device=dev)
    hist[:len(history)] = ti(history)
    d_ch, d_dr, d_tok, d_rp = ti(chosen), ti(drafts), torch.full((k + 1,), -1, dtype=torch.int32, device=dev), torch.full((k + 1,), -1, dtype=torch.int32, device=dev)
    d_pos, d_rem, d_rec = ti([pos]), ti([remaining]), torch.full((3,), -9, dtype=torch.int32, device=dev)
    st = _SpecState(ctypes.sizeof(_SpecState), k, 1, 64, 1, nmax, nmin, d_tok.data_ptr(), None, d_rp.data_ptr(), d_dr.data_ptr(), d_ch.data_ptr(),
                    d_pos.data_ptr(), d_rem.data_ptr(), hist.data_ptr(), d_rec.data_ptr(), None, None, None, None, 0)
    L.check(lib.onebit_spec_commit(ctypes.byref(st), max_len, _sp()), "spec_commit")
    torch.cuda.synchronize()
    rec = d_rec.tolist()
    return dict(n_acc=rec[0], pos=int(d_pos[0]), rec_pos=rec[1], n_drafted=rec[2], remaining=int(d_rem[0]), history=hist.tolist(),
                tokens=d_tok.tolist(), row_pos=d_rp.tolist(), drafts=d_dr.tolist())


def _check_commit(got, ref, max_len, n_hist):
    assert got["n_acc"] == ref["n_acc"] and got["pos"] == ref["pos"] == got["rec_pos"] and got["n_drafted"] == ref["n_drafted"]
    assert got["remaining"] == ref["remaining"]
    assert got["history"][:ref["pos"] + 1] == ref["history"]
    assert all(t == -7 for t in got["history"][max(ref["pos"] + 1, n_hist):])              # nothing written past the emitted tokens
    assert got["tokens"] == ref["tokens"] and got["row_pos"] == ref["row_pos"] and got["drafts"] == ref["drafts"]


def test_commit_kernel_equals_the_reference_exactly():
    L, lib = _lib()
    rng = np.random.default_rng(42)
    cases = 0
    for max_len in (16, 64, 1000, 4096):
        for vocab in (2, 3, 7):
            for _ in range(6):
                k = int(rng.integers(1, 16))
                n = int(rng.integers(1, max_len + 1)) if rng.random() < 0.7 else int(rng.integers(max(1, max_len - 8), max_len + 1))
                history = rng.integers(0, vocab, n).tolist()
                pos = n - 1
                drafts = rng.integers(0, vocab, k).tolist()
                chosen = rng.integers(0, vocab, k + 1).tolist()
                j = int(rng.integers(0, k + 1))
                chosen[:j] = drafts[:j]                                             # accept a prefix of random length
                remaining = int(rng.integers(0, 4)) if rng.random() < 0.3 else 1000
                nmin = int(rng.integers(1, 3))
                nmax = int(rng.integers(nmin, 6))
                ref = commit_ref(chosen, drafts, pos, remaining, history, max_len, nmax, nmin)
                got = _commit(lib, L, chosen, drafts, pos, remaining, history, max_len, nmax, nmin)
                _check_commit(got, ref, max_len, n)
                cases += 1
    # the hand-written histories of the CPU test through the kernel; the caps by hand
    for history, k, nmax, nmin in [([1, 2, 3, 4], 3, 3, 1), ([5, 6, 7, 8, 9, 5, 6], 3, 2, 2), ([1, 1, 1, 1], 3, 3, 1), ([1, 2, 1, 2, 1], 4, 3, 1),
                                   ([3, 4, 9, 3, 4], 5, 2, 1), ([1, 2, 5, 0, 1, 2, 6, 0, 1], 1, 2, 2), ([4, 8, 1, 9, 2], 2, 3, 1), ([4, 8, 1, 9, 2], 2, 3, 2)]:
        # the last token of each case arrives as chosen[0] of a step that accepts nothing
        h, c0 = history[:-1], history[-1] if len(history) > 1 else history[0]
        drafts, chosen = [c0 + 1] * k, [c0] + [0] * k
        ref = commit_ref(chosen, drafts, len(h) - 1, 50, h, 64, nmax, nmin)
        assert ref["n_acc"] == 0
        _check_commit(_commit(lib, L, chosen, drafts, len(h) - 1, 50, h, 64, nmax, nmin), ref, 64, len(h))
    full = commit_ref([1, 2, 3, 4], [1, 2, 3], 4095 - 2, 100, [0] * (4096 - 2), 4096, 3, 1)
    assert full["n_acc"] == 1 and full["pos"] == 4095
    _check_commit(_commit(lib, L, [1, 2, 3, 4], [1, 2, 3], 4095 - 2, 100, [0] * (4096 - 2), 4096, 3, 1), full, 4096, 4094)
    none = commit_ref([1, 2], [1], 63, 5, [3] * 64, 64, 3, 1)
    assert none["n_acc"] == -1
    _check_commit(_commit(lib, L, [1, 2], [1], 63, 5, [3] * 64, 64, 3, 1), none, 64, 64)
    assert cases == 72


# ---------------------------------------------------------------------------------------------- multi-query attention --
@pytest.mark.parametrize("H,Hkv,D,chunk,max_len,nsplit", [
    (4, 4, 64, 64, 400, None), (8, 2, 128, 128, 1100, None), (32, 32, 128, 128, 2048, None), (8, 2, 64, 192, 700, None),
    (4, 2, 128, 128, 128, 1), (4, 4, 64, 64, 64, 1)])
@pytest.mark.parametrize("Q", [2, 5, 16])
@pytest.mark.parametrize("use_h", [False, True])
def test_mq_attention_is_the_single_row_kernel_bit_for_bit(H, Hkv, D, chunk, max_len, nsplit, Q, use_h):
    L, lib = _lib()
    dev = torch.device(DEV)
    g = torch.Generator(device="cpu").manual_seed(11 + chunk + Q)
    # first positions: 0; rows straddling a chunk boundary (rows with different nlive); inside a chunk; the end of the cache (idle tail rows)
    first = [0, chunk - 2, chunk - Q + 1 if chunk > Q else 1, 2 * chunk - 1, 3 * chunk + 5, max_len - Q, max_len - 2, max_len // 2]
    first = sorted({p for p in first if 0 <= p < max_len})
    if nsplit is None:
        nsplit = -(-max_len // chunk)
    n_seq = len(first)
    slots = n_seq + 1
    slot_of = [slots - 1 - i for i in range(n_seq)]
    assert len(set(slot_of)) == n_seq
    rows = n_seq * Q
    q = torch.randn(rows, H, D, generator=g).half().to(dev)
    kc = (torch.randn(slots, Hkv, max_len, D, generator=g) * 0.7).half().to(dev)
    vc = torch.randn(slots, Hkv, max_len, D, generator=g).half().to(dev)
    h_next = (0.5 + torch.rand(H * D, generator=g)).half().to(dev) if use_h else None
    hp = h_next.data_ptr() if use_h else None
    row_slot = torch.tensor([s for s in slot_of for _ in range(Q)], dtype=torch.int32, device=dev)
    row_pos = torch.tensor([p + i for p in first for i in range(Q)], dtype=torch.int32, device=dev)
    nb = int(lib.onebit_attention_decode_scratch_bytes(rows, H, nsplit))
    scr_a = torch.zeros(max(nb, 16), dtype=torch.uint8, device=dev)
    scr_b = torch.zeros(max(nb, 16), dtype=torch.uint8, device=dev)
    ref = torch.full((rows, H * D), 9.0, dtype=torch.float16, device=dev)
    L.check(lib.onebit_attention_decode_rows(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ref.data_ptr(), hp, row_slot.data_ptr(), row_pos.data_ptr(),
                                             rows, H, Hkv, D, slots, max_len, chunk, nsplit, scr_a.data_ptr(), scr_a.numel(), _sp()), "fdec")
    outs = []
    for rep in range(3):
        o = torch.full((rows, H * D), 9.0, dtype=torch.float16, device=dev)
        L.check(lib.onebit_attention_decode_rows_mq(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), hp, row_slot.data_ptr(), row_pos.data_ptr(),
                                                    rows, Q, H, Hkv, D, slots, max_len, chunk, nsplit, scr_b.data_ptr(), scr_b.numel(), _sp()), "fdec_mq")
        torch.cuda.synchronize()
        outs.append(o)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    if nb:
        assert int(scr_b[:rows * H * 4].max()) == 0                                   # every ticket word reads zero
    live = (row_pos < max_len).cpu()
    assert bool(live.any()) and not bool(torch.isnan(outs[0][live.to(dev)].float()).any())
    assert float((outs[0][(~live).to(dev)].float() - 9.0).abs().max() if bool((~live).any()) else 0.0) == 0.0     # rows beyond the cache untouched
    bad = (outs[0] != ref).any(dim=1).nonzero().flatten().tolist()
    assert torch.equal(outs[0], ref), ("rows that differ", bad[:8], [int(row_pos[r]) for r in bad[:8]])


def test_mq_attention_with_a_grid_that_does_not_cover_the_context():
    """The clamp the new kernel applies (nlive = min(ceil(L / chunk), nsplit)): every row is written from the keys the grid covers and
    the tickets return to zero."""
    L, lib = _lib()
    dev = torch.device(DEV)
    g = torch.Generator(device="cpu").manual_seed(3)
    H, D, chunk, max_len, Q, nsplit = 4, 64, 64, 400, 5, 2
    q = torch.randn(Q, H, D, generator=g).half().to(dev)
    kc = torch.randn(1, H, max_len, D, generator=g).half().to(dev)
    vc = torch.randn(1, H, max_len, D, generator=g).half().to(dev)
    pos0 = 300
    row_pos = torch.arange(pos0, pos0 + Q, dtype=torch.int32, device=dev)
    nb = int(lib.onebit_attention_decode_scratch_bytes(Q, H, nsplit))
    scr = torch.zeros(nb, dtype=torch.uint8, device=dev)
    o = torch.full((Q, H * D), 9.0, dtype=torch.float16, device=dev)
    L.check(lib.onebit_attention_decode_rows_mq(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), None, None, row_pos.data_ptr(),
                                                Q, Q, H, H, D, 1, max_len, chunk, nsplit, scr.data_ptr(), scr.numel(), _sp()), "fdec_mq")
    torch.cuda.synchronize()
    assert int(scr[:Q * H * 4].max()) == 0
    s = torch.einsum("qhd,hld->hql", q.float(), kc[0, :, :nsplit * chunk].float()) / 8.0
    ref = torch.einsum("hql,hld->qhd", torch.softmax(s, -1), vc[0, :, :nsplit * chunk].float()).reshape(Q, H * D)
    assert float((o.float() - ref).abs().max()) < 4e-3


# -------------------------------------------------------------------------------------------------------------- models --
def _tiny(golden_dir, name, dev):
    from onebit_amd.llama import OneBitLlamaConfig, OneBitLlamaForCausalLM
    z = np.load(os.path.join(golden_dir, f"model_tiny_{name}.npz"))
    kw = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg_")}
    model = OneBitLlamaForCausalLM(OneBitLlamaConfig(**kw), torch.float16)
    model.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")})
    return z, model.to(dev).eval()


def _wide(golden_dir, name, dev):
    from onebit_amd.llama import OneBitLlamaConfig, OneBitLlamaForCausalLM, synthetic_state_dict
    z = np.load(os.path.join(golden_dir, f"model_wide_{name}.npz"))
    kw = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg_")}
    cfg = OneBitLlamaConfig(**kw)
    model = OneBitLlamaForCausalLM(cfg, torch.float16)
    model.load_state_dict(synthetic_state_dict(cfg, seed=int(z["seed"]), dtype=torch.float16, device="cpu"))
    return z, model.to(dev).eval()


def _load(golden_dir, name, dev):
    return _wide(golden_dir, name[5:], dev) if name.startswith("wide_") else _tiny(golden_dir, name[5:], dev)


def _near_tie(model, p, ref, got, dev):
    """tests/test_gpu_mixed.py's rule: at the first difference the module path's logits of the two tokens lie within 2e-2 x the logit scale."""
    j = next(i for i in range(len(ref)) if got[i] != ref[i])
    lg = model(torch.tensor([p + ref[:j]], device=dev))[0, -1]
    return abs(float(lg[got[j]] - lg[ref[j]])) < 2e-2 * float(lg.abs().max())


def _same_tokens(test, model, prompt, ref, got, dev, allow_tie):
    assert len(got) == len(ref), (test, len(got), len(ref))
    if got == ref:
        return
    assert allow_tie, (test, "tokens differ on a tiny fixture", ref, got)
    assert _near_tie(model, prompt, ref, got, dev), (test, ref, got)
    NEAR_TIE_USES.append((test, next(i for i in range(len(ref)) if got[i] != ref[i])))
    print(f"near-tie rule used: {test} (uses so far: {len(NEAR_TIE_USES)})")


# ------------------------------------------------------------------------------ the verify pass against the reference --
@pytest.mark.parametrize("name", ["wide_c", "wide_e", "tiny_bias"])
def test_verify_pass_logits_against_the_reference_teacher_forced(golden_dir, name):
    from _parity_log import loose_tol
    from onebit_amd.engine import DecodeEngine, SpecStep
    from onebit_amd.speculative import SpecConfig
    dev = torch.device(DEV)
    z, model = _load(golden_dir, name, dev)
    ids, greedy = z["input_ids"][0].tolist(), z["greedy_f16"][0].tolist()
    S, G = len(ids), len(greedy)
    seq = ids + greedy                                    # the golden sequence; the reference's logits exist at positions 0 .. S + G - 2
    ref16 = np.concatenate([z["prefill_logits_f16"][0], z["decode_logits_f16"][0]], axis=0).astype(np.float32)
    ref32 = np.concatenate([z["prefill_logits_f32"][0], z["decode_logits_f32"][0]], axis=0).astype(np.float32)
    tol = max(loose_tol(z["prefill_logits_f16"], z["prefill_logits_f32"]), loose_tol(z["decode_logits_f16"], z["decode_logits_f32"]))
    k = G - 1                                             # the last step's drafts are the reference's greedy continuation
    p0 = (S - 1) % (k + 1)
    assert p0 >= 1
    eng = DecodeEngine(model, max_len=32)
    eng.prime(torch.tensor([ids[:p0]], device=dev))
    spec = SpecStep(eng.model, eng.cache.layers, 1, 32, SpecConfig(k), keep_logits=True)
    worst16 = worst32 = 0.0
    for p in range(p0, S, k + 1):
        spec.seed(seq[:p + 1], remaining=k + 1, drafts=seq[p + 1:p + 1 + k])
        spec.step()
        n_acc, pos, _ = spec.read_record()
        lg = spec.logits.float().cpu().numpy()
        e16, e32 = float(np.abs(lg - ref16[p:p + k + 1]).max()), float(np.abs(lg - ref32[p:p + k + 1]).max())
        print(f"{name}: rows {p}..{p + k}: max |dlogit| vs fp16 {e16:.5f}, vs fp32 {e32:.5f}, bar {tol:.5f}, n_acc {n_acc}")
        worst16, worst32 = max(worst16, e16), max(worst32, e32)
        assert e16 <= tol and e32 <= tol, (name, p, e16, e32, tol)
        assert spec.chosen.tolist() == lg.argmax(-1).tolist()
        if p == S - 1:                                    # drafts = the reference's own greedy tokens: every one accepted
            assert n_acc == k and pos == p + k + 1, (n_acc, pos)
            assert spec.history[S:S + G].tolist() == greedy


# ------------------------------------------------------------------------------------------------- end to end, greedy --
def _repeating_prompt(V, seed):
    g = torch.Generator().manual_seed(seed)
    span = torch.randint(0, V, (6,), generator=g).tolist()
    return span + torch.randint(0, V, (3,), generator=g).tolist() + span + span


def _well_conditioned_repeating_prompt(model, V, n, dev, strict):
    """The first seed (7, 8, ...) whose prompt the MODULE PATH (the comparison's reference side, not the code under test) decodes
    (a) into a continuation that prompt lookup predicts at least once (host ``propose`` / ``accept`` on the module path's tokens) and,
    with ``strict`` (the tiny fixtures, where no near-tie use is allowed), (b) with every greedy token ahead of the runner-up by at
    least 16 fp16 ulps of the logit scale.  Why (b): the engine's GEMV route and the speculative step's skinny-GEMM route sum in
    different orders and each lies within a few ulps of the reference (tests/_parity_log: 2e-3 x scale and up, i.e. >= 4 ulps), so
    only a margin of several times that makes 'the same argmax' a property of the input instead of a coin toss.  Seed 7 on
    model_tiny_b is such a toss: at its 19th token the module path's two best logits are 0.52930 and 0.52881, ONE fp16 ulp apart,
    the engine takes one and the mixed-step route the other (measured; speculative tokens == one-token-at-a-time tokens through the
    same step there, which the test asserts for every prompt)."""
    from onebit_amd.speculative import accept, propose
    for seed in range(7, 40):
        prompt = _repeating_prompt(V, seed)
        full = model.generate(torch.tensor([prompt], device=dev), n)[0]
        lg = model(full[None, :-1])[0, len(prompt) - 1:].float()
        top = torch.topk(lg, 2, dim=-1).values
        scale = float(lg.abs().max())
        ulp = 2.0 ** (np.floor(np.log2(scale)) - 10)
        if strict and float((top[:, 0] - top[:, 1]).min()) < 16 * ulp:
            continue
        toks, acc, i = full.tolist(), 0, len(prompt) + 1
        while i < len(toks):
            d = propose(toks[:i], 4)[0]
            a = accept(d[:len(toks) - i - 1], toks[i:i + 5]) if len(toks) - i > 1 else 0
            acc, i = acc + a, i + a + 1
        if acc > 0:
            print(f"repeating prompt: seed {seed}, module-path acceptance at k = 4: {acc} drafts")
            return prompt
    raise AssertionError("no well-conditioned repeating prompt among seeds 7 .. 39")


# (model_tiny_a is not here: its intermediate size 688 is no multiple of 32 and the decode engines refuse it, with or without speculation)
@pytest.mark.parametrize("name", ["tiny_b", "tiny_bias", "wide_c", "wide_e"])
def test_generate_speculative_equals_generate_greedy(golden_dir, name):
    from onebit_amd.engine import DecodeEngine
    from onebit_amd.speculative import SpecConfig
    dev = torch.device(DEV)
    z, model = _load(golden_dir, name, dev)
    tiny = name.startswith("tiny")
    V = model.config.vocab_size
    max_len = 64
    eng = DecodeEngine(model, max_len=max_len)
    golden = z["input_ids"][0].tolist()
    accepted = 0
    for kind, prompt, n in (("golden", golden, 12), ("repeat", _well_conditioned_repeating_prompt(model, V, 40, dev, tiny), 40),
                            ("repeat, seed 7", _repeating_prompt(V, 7), 40)):
        ids = torch.tensor([prompt], device=dev)
        ref = eng.generate(ids, n)[0, len(prompt):].tolist()
        for k in (1, 4, 8):
            got = eng.generate(ids, n, speculative=SpecConfig(k))[0, len(prompt):].tolist()
            recs = list(eng.spec_records)
            # speculation itself is exact, on every prompt: the tokens of one-token-at-a-time decoding through the same step
            # (drafts that are never accepted), whatever the summation order of that step does to a near-tie
            never = next(t for t in range(V) if t not in got)
            assert got == eng.generate(ids, n, speculative=SpecConfig(k), drafts=lambda m: [never] * k)[0, len(prompt):].tolist()
            if kind == "repeat, seed 7":
                continue                      # an ill-conditioned input for the cross-route comparison (see _well_conditioned_repeating_prompt)
            _same_tokens(f"{name}/{kind}/k{k}", model, prompt, ref, got, dev, allow_tie=not tiny)
            assert sum(r[0] + 1 for r in recs) == n - 1 and all(0 <= r[0] <= k for r in recs)
            if kind == "repeat":
                accepted += sum(r[0] for r in recs)
                print(f"{name}/{kind}/k{k}: {len(recs)} steps for {n - 1} tokens, accepted drafts per step {[r[0] for r in recs]}")
            # oracle drafts: the plain run's tokens -> every draft accepted, ceil((n - 1) / (k + 1)) steps
            full = prompt + ref
            oracle = lambda m, k=k: (full[m:m + k] + [0] * k)[:k]
            got = eng.generate(ids, n, speculative=SpecConfig(k), drafts=oracle)[0, len(prompt):].tolist()
            if got == ref:
                assert len(eng.spec_records) == -(-(n - 1) // (k + 1)), eng.spec_records
            _same_tokens(f"{name}/{kind}/k{k}/oracle", model, prompt, ref, got, dev, allow_tie=not tiny)
            # adversarial drafts: a token the plain run never emits -> n_acc = 0 in every step; the rejected rows' keys / values are
            # overwritten by the next step before anything attends to them
            bad = next(t for t in range(V) if t not in ref)
            got = eng.generate(ids, n, speculative=SpecConfig(k), drafts=lambda m: [bad] * k)[0, len(prompt):].tolist()
            if got == ref:
                assert all(r[0] == 0 for r in eng.spec_records) and len(eng.spec_records) == n - 1
            _same_tokens(f"{name}/{kind}/k{k}/adversarial", model, prompt, ref, got, dev, allow_tie=not tiny)
    # the repeating prompt makes greedy output cycle on these small models: without an accepted draft this proves nothing
    assert accepted > 0, "no draft was ever accepted"
    # a run that ends exactly at the last cache position
    prompt = golden
    n = max_len - len(prompt)
    ids = torch.tensor([prompt], device=dev)
    ref = eng.generate(ids, n)[0, len(prompt):].tolist()
    for k in (4, 8):
        got = eng.generate(ids, n, speculative=SpecConfig(k))[0, len(prompt):].tolist()
        assert eng.spec_records[-1][1] == max_len - 1
        _same_tokens(f"{name}/to max_len/k{k}", model, prompt, ref, got, dev, allow_tie=not tiny)
    # the engine goes on one token at a time from where the speculative run stopped
    got = eng.generate(ids, 10, speculative=SpecConfig(4))
    eng.step()
    torch.cuda.synchronize()
    assert int(eng.token[0]) == ref[10] or not tiny
    print("near-tie uses:", NEAR_TIE_USES)


def test_generate_speculative_across_the_keyblock_handover_and_a_growing_split_count(golden_dir):
    """model_wide_c, max_len 512, attention chunks of 128 keys: a prompt of 150 tokens and 130 new ones cross position 160 (where the plain
    engine hands over from the one-workgroup attention to the key-block graphs) and 256 (2 -> 4 splits, a second captured graph)."""
    from onebit_amd.engine import DecodeEngine
    from onebit_amd.speculative import SpecConfig
    dev = torch.device(DEV)
    z, model = _wide(golden_dir, "c", dev)
    V = model.config.vocab_size
    eng = DecodeEngine(model, max_len=512)
    g = torch.Generator().manual_seed(19)
    span = torch.randint(0, V, (10,), generator=g).tolist()
    prompt = torch.randint(0, V, (120,), generator=g).tolist() + span + span + span
    ids = torch.tensor([prompt], device=dev)
    n = 130
    ref = eng.generate(ids, n)[0, len(prompt):].tolist()
    for k in (4, 8):
        got = eng.generate(ids, n, speculative=SpecConfig(k))[0, len(prompt):].tolist()
        spec = eng._spec_steps[(k, 3, 1)]
        assert spec.attn_chunk == 128 and {ns for (ns, _, _) in spec._seen} >= {2, 4}
        assert eng.spec_records[0][1] > 150 and eng.spec_records[-1][1] == len(prompt) + n - 1
        print(f"k{k}: {len(eng.spec_records)} steps for {n - 1} tokens")
        _same_tokens(f"wide_c/handover/k{k}", model, prompt, ref, got, dev, allow_tie=True)
        full = prompt + ref
        got = eng.generate(ids, n, speculative=SpecConfig(k), drafts=lambda m, k=k: (full[m:m + k] + [0] * k)[:k])[0, len(prompt):].tolist()
        _same_tokens(f"wide_c/handover/k{k}/oracle", model, prompt, ref, got, dev, allow_tie=True)
    print("near-tie uses:", NEAR_TIE_USES)


# ------------------------------------------------------------------------------------------------ end to end, sampled --
def _perturbed(model, prefix, n, sp, dev):
    """The module path's fp32 scores + the sampler's Gumbel noise at token n (tests/_sampling_ref.py)."""
    from _sampling_ref import gumbel, scores
    lg = model(torch.tensor([prefix], device=dev))[0, -1].half().cpu().numpy()
    s = scores(lg, sp.temperature).astype(np.float64)
    return s + gumbel(len(s), sp.seed & 0xFFFFFFFF, sp.seed >> 32, sp.stream, n)


@pytest.mark.parametrize("name", ["tiny_b", "tiny_bias"])
def test_generate_speculative_equals_generate_sampled(golden_dir, name):
    from onebit_amd.engine import DecodeEngine
    from onebit_amd.sampling import SamplingParams
    from onebit_amd.speculative import SpecConfig
    dev = torch.device(DEV)
    z, model = _tiny(golden_dir, name[5:], dev)
    V = model.config.vocab_size
    sp = SamplingParams(temperature=0.8, top_k=50, top_p=0.9, seed=1)
    eng = DecodeEngine(model, max_len=64)
    for kind, prompt, n in (("golden", z["input_ids"][0].tolist(), 20), ("repeat", _repeating_prompt(V, 7), 36)):
        ids = torch.tensor([prompt], device=dev)
        ref = eng.generate(ids, n, sampling=sp)[0, len(prompt):].tolist()
        full = prompt + ref
        for k in (1, 4, 8):
            for drafts in (None, lambda m, k=k: (full[m:m + k] + [0] * k)[:k]):
                got = eng.generate(ids, n, sampling=sp, speculative=SpecConfig(k), drafts=drafts)[0, len(prompt):].tolist()
                if drafts is not None and got == ref:
                    assert all(r[0] == min(k, n - 1) or r is eng.spec_records[-1] for r in eng.spec_records)     # every draw confirmed its draft
                if got != ref:
                    j = next(i for i in range(n) if got[i] != ref[i])
                    sc = _perturbed(model, prompt + ref[:j], len(prompt) + j, sp, dev)       # token j is drawn at n = its index in the sequence
                    assert abs(sc[got[j]] - sc[ref[j]]) < 2e-2 * max(1.0, float(np.abs(sc[np.isfinite(sc)]).max())), (name, kind, k, j)
                    NEAR_TIE_USES.append((f"{name}/{kind}/k{k}/sampled", j))
                    print(f"near-tie rule used (sampled): {name}/{kind}/k{k} at token {j} (uses so far: {len(NEAR_TIE_USES)})")
    print("near-tie uses:", NEAR_TIE_USES)


# --------------------------------------------------------------------------- speculative=None: the parent's launches --
def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    import tempfile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "trace.json")
        prof.export_chrome_trace(path)
        with open(path) as f:
            events = json.load(f).get("traceEvents", [])
    ks = [(e.get("ts", 0), e.get("name", ""), str(e.get("args", {}).get("grid")), str(e.get("args", {}).get("block")))
          for e in events if str(e.get("cat", "")).lower() == "kernel"]
    return [k[1:] for k in sorted(ks)]


def test_generate_without_speculation_launches_what_it_did_before(golden_dir):
    """The expected list is derived from the non-speculative engine in the same process: prime() + (n - 1) x step() is the body
    generate() had before it learnt ``speculative=`` (with the concatenation that builds its return value); name, grid and block of every dispatch, in order, as tests/route_switch_child.py
    records them.  Run before and after a speculative generate on the same engine (it leaves nothing behind that changes the path)."""
    from onebit_amd.engine import DecodeEngine
    from onebit_amd.speculative import SpecConfig
    dev = torch.device(DEV)
    z, model = _tiny(golden_dir, "b", dev)
    ids = torch.tensor(z["input_ids"], device=dev)
    eng = DecodeEngine(model, max_len=64)
    n = 9

    def parent():
        eng.prime(ids)
        for _ in range(n - 1):
            eng.step()
        torch.cuda.synchronize(dev)
        new = [eng.first_token] + eng.out_tokens[eng._prompt_len:eng._prompt_len + n - 1].tolist()
        torch.cat([ids, torch.tensor([new], device=dev, dtype=ids.dtype)], dim=1)

    parent()
    torch.cuda.synchronize()                                    # (first use allocates the prefill workspace)
    want = _launches(parent)
    assert len(want) > 8 * (n - 1)
    assert _launches(lambda: eng.generate(ids, n, speculative=None)) == want
    assert _launches(lambda: eng.generate(ids, n)) == want
    spec = _launches(lambda: eng.generate(ids, n, speculative=SpecConfig(4)))
    assert any("ob_fdec_mq_kernel" in k[0] for k in spec) and any("ob_spec_commit_kernel" in k[0] for k in spec)
    assert not any("ob_fdec_mq_kernel" in k[0] or "ob_spec" in k[0] for k in want)
    assert _launches(lambda: eng.generate(ids, n, speculative=None)) == want
