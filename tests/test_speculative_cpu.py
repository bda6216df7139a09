"""Speculative decoding, the parts that need no GPU: the host statement of the commit contract (onebit_amd/speculative.py)
against the numpy restatement in tests/_spec_ref.py, and the C entry points' argument checks (no launch is reached)."""
import ctypes

import numpy as np
import pytest

from _spec_ref import accept_ref, commit_ref, propose_ref
from onebit_amd import _lib
from onebit_amd.speculative import SpecConfig, accept, propose


@pytest.mark.parametrize("vocab", [2, 3, 5, 11])
def test_propose_and_accept_on_random_histories(vocab):
    rng = np.random.default_rng(100 + vocab)
    matched = 0
    for _ in range(400):
        n = int(rng.integers(1, 60))
        h = rng.integers(0, vocab, n).tolist()
        k = int(rng.integers(1, 16))
        nmin = int(rng.integers(1, 4))
        nmax = int(rng.integers(nmin, 6))
        got = propose(h, k, nmax, nmin)
        assert (list(got[0]), got[1]) == propose_ref(h, k, nmax, nmin), (h, k, nmax, nmin)
        assert len(got[0]) == k and 0 <= got[1] <= k
        matched += got[1] > 0
        d = rng.integers(0, vocab, k).tolist()
        c = rng.integers(0, vocab, k + 1).tolist()
        if rng.random() < 0.5:
            j = int(rng.integers(0, k + 1))
            c[:j] = d[:j]
        assert accept(d, c) == accept_ref(d, c)
    assert matched > 100                      # small vocabularies: the lookup finds something most of the time


def test_propose_hand_written_cases():
    # no match: every slot repeats the last token
    assert propose([1, 2, 3, 4], 3) == ([4, 4, 4], 0)
    assert propose([7], 2) == ([7, 7], 0)
    # match at the very start of the history
    assert propose([5, 6, 7, 8, 9, 5, 6], 3, 2, 2) == ([7, 8, 9], 3)
    # overlapping match: the occurrence overlaps the suffix itself; only history can follow
    assert propose([1, 1, 1, 1], 3, 3, 1) == ([1, 1, 1], 1)
    assert propose([1, 2, 1, 2, 1], 4, 3, 1) == ([2, 1, 1, 1], 2)
    # fewer followers than k: the remaining slots repeat the last token
    assert propose([3, 4, 9, 3, 4], 5, 2, 1) == ([9, 3, 4, 4, 4], 3)
    # the latest occurrence wins
    assert propose([1, 2, 5, 0, 1, 2, 6, 0, 1, 2], 1, 2, 2) == ([6], 1)
    # ngram_min fallback: no 3- or 2-gram repeats, the 1-gram does; and ngram_min = 2 refuses it
    assert propose([4, 8, 1, 9, 2, 8], 2, 3, 1) == ([1, 9], 2)
    assert propose([4, 8, 1, 9, 2, 8], 2, 3, 2) == ([8, 8], 0)
    # the longest n-gram is preferred over a later shorter one
    assert propose([1, 2, 3, 7, 0, 3, 8, 1, 2, 3], 1, 3, 1) == ([7], 1)
    for case in ([1, 2, 3, 4], [5, 6, 7, 8, 9, 5, 6], [1, 1, 1, 1], [1, 2, 1, 2, 1], [3, 4, 9, 3, 4], [4, 8, 1, 9, 2, 8]):
        for k in (1, 3, 5):
            for nmax, nmin in ((3, 1), (2, 2), (1, 1)):
                got = propose(case, k, nmax, nmin)
                assert (list(got[0]), got[1]) == propose_ref(case, k, nmax, nmin)
    assert accept([1, 2, 3], [1, 2, 3, 4]) == 3 and accept([1, 2, 3], [1, 9, 3, 4]) == 1 and accept([5], [6, 5]) == 0


def test_commit_ref_caps():
    """The restatement's own caps, by hand: the budget and the end of the cache."""
    r = commit_ref([1, 2, 3, 4], [1, 2, 3], pos=4, remaining=2, history=[9, 9, 9, 9, 0], max_len=64, ngram_max=3, ngram_min=1)
    assert (r["n_acc"], r["pos"], r["remaining"]) == (1, 6, 0) and r["history"][-2:] == [1, 2]
    r = commit_ref([1, 2, 3, 4], [1, 2, 3], pos=5, remaining=9, history=[9] * 6, max_len=8, ngram_max=3, ngram_min=1)
    assert (r["n_acc"], r["pos"]) == (1, 7)                   # pos + n_acc + 1 < max_len
    r = commit_ref([1, 2], [1], pos=7, remaining=9, history=[9] * 8, max_len=8, ngram_max=3, ngram_min=1)
    assert (r["n_acc"], r["pos"], r["remaining"]) == (-1, 7, 9)


def test_spec_config_validates():
    assert SpecConfig(4).ngram_max == 3 and SpecConfig(4).ngram_min == 1
    for bad in (dict(draft_tokens=0), dict(draft_tokens=16), dict(draft_tokens=2, ngram_min=0), dict(draft_tokens=2, ngram_max=1, ngram_min=2)):
        with pytest.raises(ValueError):
            SpecConfig(**bad)


def test_spec_entry_points_exported_and_reject_bad_arguments_without_gpu():
    lib = _lib.load()
    for name in ("onebit_spec_step", "onebit_spec_step_sampled", "onebit_spec_workspace_bytes", "onebit_attention_decode_rows_mq"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert lib.onebit_abi_version() == 10
    E_ARG, E_SHAPE, E_WSPACE = -1, -2, -5
    from onebit_amd.engine import _Layer, _Model, _SpecState
    buf = ctypes.create_string_buffer(8192)
    a = (ctypes.addressof(buf) + 255) & ~255
    layers = (_Layer * 1)()
    m = _Model(1, 64, 128, 1, 1, 64, 16, 32, 1e-6, 1e-5, layers, a, a, a, a, a)
    assert lib.onebit_spec_workspace_bytes(ctypes.byref(m), 0, 64) == 0 and lib.onebit_spec_workspace_bytes(ctypes.byref(m), 16, 64) == 0
    need = lib.onebit_spec_workspace_bytes(ctypes.byref(m), 4, 64)
    assert need > 0 and lib.onebit_spec_workspace_bytes(ctypes.byref(m), 8, 64) > need

    def state(**kw):
        st = _SpecState(ctypes.sizeof(_SpecState), kw.get("k", 4), 1, kw.get("chunk", 64), kw.get("ns", 1), kw.get("nmax", 3), kw.get("nmin", 1),
                        kw.get("tokens", a), a, a, a, a, a, a, kw.get("history", a), a, kw.get("logits", None), a, a, kw.get("ws", a),
                        kw.get("nb", need))
        st.struct_size = kw.get("size", ctypes.sizeof(_SpecState))
        return st

    def step(**kw):
        st = state(**kw)                                        # (kept alive across the call)
        return lib.onebit_spec_step(ctypes.byref(m), ctypes.byref(st), None)

    assert lib.onebit_spec_step(None, None, None) == E_ARG
    assert step(k=0) == E_ARG and b"draft" in lib.onebit_last_error()
    assert step(k=16) == E_ARG
    assert step(size=ctypes.sizeof(_SpecState) - 8) == E_ARG and b"struct_size" in lib.onebit_last_error()
    assert step(tokens=None) == E_ARG and step(history=None) == E_ARG and step(ws=None) == E_ARG
    assert step(chunk=96) == E_SHAPE and step(ns=0) == E_SHAPE and step(ns=65) == E_SHAPE
    assert step(nmin=0) == E_ARG and step(nmax=2, nmin=3) == E_ARG
    assert step(k=8) == E_WSPACE                                # the scratch holds 5 rows, the step has 9
    assert step(nb=need - 1) == E_WSPACE
    def prm(**kw):
        st = state(**kw)
        return lib.onebit_spec_step_sampled(ctypes.byref(m), ctypes.byref(st), kw.get("params", a), None)

    assert prm(params=None) == E_ARG and prm() == E_ARG and b"logits" in lib.onebit_last_error()
    assert prm(k=16, logits=a) == E_ARG
    # the multi-query attention: rows per sequence 1 .. 16 dividing the rows; the single-row entry point's checks otherwise
    mq = lambda **kw: lib.onebit_attention_decode_rows_mq(a, a, a, a, None, None, kw.get("pos", a), kw.get("rows", 4), kw.get("q", 2), 4, kw.get("hkv", 4),
                                                          kw.get("D", 64), 4, 16, kw.get("chunk", 64), kw.get("ns", 1), None, 0, None)
    assert mq(q=0) == E_SHAPE and mq(q=17, rows=17) == E_SHAPE and mq(q=3) == E_SHAPE
    assert mq(chunk=96) == E_SHAPE and mq(D=12) == E_SHAPE and mq(hkv=3) == E_SHAPE and mq(ns=3) == E_WSPACE
    assert mq(pos=None) == E_ARG and mq(rows=0) == 0
    assert lib.onebit_spec_commit(None, 64, None) == E_ARG
    st = state()
    assert lib.onebit_spec_commit(ctypes.byref(st), 20000, None) == E_SHAPE


def test_generate_native_refuses_speculative_batches():
    import torch
    from onebit_amd.llama import OneBitLlamaConfig, OneBitLlamaForCausalLM
    cfg = OneBitLlamaConfig(vocab_size=32, hidden_size=64, intermediate_size=96, num_hidden_layers=1, num_attention_heads=1,
                            max_position_embeddings=32)
    model = OneBitLlamaForCausalLM(cfg, torch.float16)
    with pytest.raises(NotImplementedError, match="B = 1"):
        model.generate_native(torch.zeros(2, 3, dtype=torch.long), 4, speculative=SpecConfig(2))
