"""CPU checks of sampled decoding (ABI 10): the test-side Philox and contract restatement, the HF warper fixture, the
SamplingParams API and its device-row layout, and the new entry points' argument errors (returned before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _sampling_ref import kept_set, philox4x32_10, scores
from onebit_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    """Random123's known-answer vectors of Philox4x32-10."""
    got = " ".join("%08x" % int(w) for w in philox4x32_10(ctr, key))
    assert got == want


def test_host_reference_kept_set_matches_hf_warpers():
    """The contract's kept set equals the reference's Temperature -> TopK -> TopP warpers on every fixture row."""
    d = np.load(os.path.join(HERE, "golden", "sampling_warpers.npz"))
    assert len(d["vocab"]) >= 40
    for i in range(len(d["vocab"])):
        V = int(d["vocab"][i])
        s = scores(d["logits"][i, :V], d["temperature"][i])
        keep, _ = kept_set(s, int(d["top_k"][i]), float(d["top_p"][i]))
        assert (keep == d["kept"][i, :V]).all(), (i, V, d["temperature"][i], d["top_k"][i], d["top_p"][i])


def test_sampling_params_validation_and_packing():
    from onebit_amd.sampling import SampleParamsStruct, SamplingParams, pack_host
    assert ctypes.sizeof(SampleParamsStruct) == 32
    offs = {n: getattr(SampleParamsStruct, n).offset for n, _ in SampleParamsStruct._fields_}
    assert offs == dict(do_sample=0, temperature=4, top_k=8, top_p=12, seed_lo=16, seed_hi=20, stream=24, reserved=28)
    p = SamplingParams()
    assert (p.temperature, p.top_k, p.top_p, p.stream) == (1.0, 50, 1.0, 0)          # GenerationConfig's defaults
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_k=-1), dict(top_k=2.5),
                dict(top_p=-0.1), dict(top_p=1.5), dict(seed=-1), dict(stream=2 ** 32)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    torch.manual_seed(7)
    a = SamplingParams().seed
    torch.manual_seed(7)
    assert SamplingParams().seed == a                                                  # repeatable under torch.manual_seed
    q = SamplingParams(temperature=0.7, top_k=5, top_p=0.9, seed=(3 << 32) | 11, stream=4)
    rows = pack_host([q, None]).numpy()
    assert rows.shape == (2, 32) and rows.dtype == np.uint8
    r0 = rows[0].view(np.int32)
    assert r0[0] == 1 and r0[2] == 5 and rows[0].view(np.float32)[1] == np.float32(0.7) and rows[0].view(np.float32)[3] == np.float32(0.9)
    assert list(rows[0].view(np.uint32)[4:]) == [11, 3, 4, 0]
    assert rows[1].view(np.int32)[0] == 0                                              # None: a greedy row


def test_sampling_entry_points_exported_and_reject_bad_arguments_without_gpu():
    lib = _lib.load()
    assert lib.onebit_abi_version() == _lib.ABI_VERSION == 10
    for s in ("onebit_sample_rows", "onebit_decode_step_sampled", "onebit_decode_step_batched_sampled", "onebit_mixed_step_sampled"):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    E_ARG, E_SHAPE = -1, -2
    buf = ctypes.create_string_buffer(8192)
    a = (ctypes.addressof(buf) + 255) & ~255
    rows = lambda **kw: lib.onebit_sample_rows(kw.get("lg", a), kw.get("ld", 64), kw.get("V", 64), kw.get("R", 2), kw.get("p", a),
                                               kw.get("pos", a), kw.get("out", a), None)
    assert rows(lg=None) == E_ARG and rows(p=None) == E_ARG and rows(pos=None) == E_ARG and rows(out=None) == E_ARG
    assert rows(V=0) == E_SHAPE and rows(V=65537, ld=65537) == E_SHAPE and rows(R=0) == E_SHAPE and rows(ld=10) == E_SHAPE
    from onebit_amd.engine import _BatchState, _MixedState, _Model, _State
    m = _Model()
    m.vocab = 70000
    st, bst, mst = _State(), _BatchState(), _MixedState()
    st.struct_size, bst.struct_size, mst.struct_size = ctypes.sizeof(_State), ctypes.sizeof(_BatchState), ctypes.sizeof(_MixedState)
    ref = ctypes.byref
    assert lib.onebit_decode_step_sampled(ref(m), ref(st), None, None) == E_ARG
    assert lib.onebit_decode_step_sampled(ref(m), ref(st), a, None) == E_SHAPE             # vocab beyond 65536
    assert lib.onebit_decode_step_batched_sampled(ref(m), ref(bst), None, None) == E_ARG
    assert lib.onebit_decode_step_batched_sampled(ref(m), ref(bst), a, None) == E_ARG      # next_tokens / logits missing
    bst.next_tokens = bst.logits = a
    assert lib.onebit_decode_step_batched_sampled(ref(m), ref(bst), a, None) == E_SHAPE
    assert lib.onebit_mixed_step_sampled(ref(m), ref(mst), None, None) == E_ARG
    mst.n_out = 3
    assert lib.onebit_mixed_step_sampled(ref(m), ref(mst), a, None) == E_ARG               # logits missing
    mst.logits = a
    assert lib.onebit_mixed_step_sampled(ref(m), ref(mst), a, None) == E_SHAPE
    m.vocab = 100
    assert lib.onebit_decode_step_sampled(ref(m), ref(st), a, None) == E_ARG                # no layers: rejected by the step's own checks
