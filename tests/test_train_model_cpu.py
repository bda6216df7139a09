"""CPU-only checks of the train-mode model (onebit_amd/train_model.py) and of the train-mode attention entry points.

1. tests/_train_model_ref.py (the torch-ops restatement that the GPU tests measure against) evaluated in float32 reproduces
   tests/golden/train_model_tiny.npz -- logits, hidden states, loss and gradients recorded from the reference's
   ``BitLlamaForCausalLM`` -- to float32 round-off.  The bar per tensor and metric is ``_train_ref.MARGIN x`` the distance of the
   restatement evaluated in FLOAT64 to the golden: the golden is itself a float32 evaluation, so that distance is the size of
   float32 round-off on this graph.  This pins the oracle; no GPU is involved.
2. / 3. state-dict keys and shapes: the model's are the reference's, and so are a start checkpoint's.
4. the C ABI rejects bad arguments before anything is launched.
5. CPU tensors and float32 on the hip route raise.
"""
import ctypes

import numpy as np
import pytest
import torch

import _train_model_ref as M
import _train_ref as R

from onebit_amd import _lib
from onebit_amd.llama import OneBitLlamaConfig


@pytest.mark.parametrize("record", M.RECORDS)
def test_restatement_fp32_reproduces_the_golden(record):
    gold = M.golden(record)
    cfg = M.CONFIGS[record]
    ids, labels = M.make_batch(cfg, M.SEEDS[record])
    assert int(gold["seed"]) == M.SEEDS[record]
    assert np.array_equal(gold["input_ids"], ids.numpy()) and np.array_equal(gold["labels"], labels.numpy())
    assert (labels == -100).sum() >= 3
    r32, r64 = M.reference(record, torch.float32), M.reference(record, torch.float64)
    bad = {}
    for n in M.names_of(cfg):
        g = torch.from_numpy(np.asarray(gold[n])).double().reshape(r64[n].shape)
        assert float(g.abs().max()) > 0 and bool(torch.isfinite(g).all()), n
        for metric in (R.peak, R.l2):
            got, bar = metric(r32[n], g), R.MARGIN * metric(r64[n], g)
            print(record, n, metric.__name__, "measured %.3e  bar %.3e" % (got, bar))
            if not got <= bar:
                bad[(n, metric.__name__)] = (got, bar)
    assert not bad, bad
    # float32 round-off, not a loose fit: the float64 evaluation is within 1e-4 of the golden everywhere
    assert all(R.peak(r64[n], torch.from_numpy(np.asarray(gold[n])).double().reshape(r64[n].shape)) < 1e-4 for n in M.names_of(cfg))


def _golden_keys(record):
    gold = M.golden(record)
    return {str(k): tuple(int(d) for d in s if d) for k, s in zip(gold["keys"], gold["shapes"])}


@pytest.mark.parametrize("record", M.RECORDS)
def test_state_dict_keys_and_shapes_are_the_references(record):
    from onebit_amd.train_model import OneBitLlamaForCausalLMTrain
    with torch.device("meta"):
        model = OneBitLlamaForCausalLMTrain(OneBitLlamaConfig(**M.CONFIGS[record]), dtype=torch.float32, attention="eager")
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert mine == _golden_keys(record)
    # what trains: the projections' three tensors; the norms, the embedding and lm_head are frozen as in the reference
    trainable = {k for k, p in model.named_parameters() if p.requires_grad}
    assert trainable == {str(k) for k in M.golden(record)["trainable"]}
    assert M.make_params(M.CONFIGS[record], 1).keys() == mine.keys()


@pytest.mark.parametrize("record", M.RECORDS)
def test_start_checkpoint_keys_are_the_models(record):
    """build_start_state_dict maps every projection's ``weight`` to weight / weight_scale / input_factor and copies the rest: its key
    set for a teacher of this config (decided by the keys alone, restated here from svid._PROJ_KEY -- the decomposition itself
    needs the GPU and is tested there)."""
    from onebit_amd import svid
    cfg = M.CONFIGS[record]
    teacher = ["model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"]
    for l in range(cfg["num_hidden_layers"]):
        teacher += [f"model.layers.{l}.{n}.weight" for n, _, _ in M.proj_shapes(cfg)]
        teacher += [f"model.layers.{l}.input_layernorm.weight", f"model.layers.{l}.post_attention_layernorm.weight"]
    out = set()
    for k in teacher:
        out.add(k)
        if svid._PROJ_KEY.match(k):
            out |= {k[:-len("weight")] + "weight_scale", k[:-len("weight")] + "input_factor"}
    assert sum(1 for k in teacher if svid._PROJ_KEY.match(k)) == 7 * cfg["num_hidden_layers"]
    assert out == set(_golden_keys(record))


def test_attention_train_abi_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    E_ARG, E_SHAPE, E_ALIGN, E_WSPACE = -1, -2, -3, -5
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) & ~63
    wsb = lib.onebit_attention_train_workspace_bytes

    def fwd(q=a, k=a, v=a, o=a, lse=a, B=1, S=8, H=2, Hkv=2, D=64):
        return lib.onebit_attention_train_forward(q, k, v, o, lse, B, S, H, Hkv, D, None)

    def bwd(ptrs=None, ws=a, nws=None, B=1, S=8, H=2, Hkv=2, D=64):
        p = [a] * 9 if ptrs is None else ptrs
        return lib.onebit_attention_train_backward(*p, ws, wsb(B, S, H, Hkv, D) if nws is None else nws, B, S, H, Hkv, D, None)

    for i in range(5):
        args = [a] * 5
        args[i] = None
        assert fwd(*args) == E_ARG, i
    assert b"null" in lib.onebit_last_error()
    for i in range(9):
        p = [a] * 9
        p[i] = None
        assert bwd(ptrs=p) == E_ARG, i
    assert bwd(ws=None) == E_ARG
    for f in (fwd, bwd):
        assert f(D=32) == E_SHAPE and f(D=96) == E_SHAPE and f(D=256) == E_SHAPE
        assert f(H=3, Hkv=2) == E_SHAPE
        assert f(B=-1) == E_ARG and f(S=-1) == E_ARG and f(H=0, Hkv=0) == E_ARG and f(H=-2) == E_ARG
        assert f(B=0) == 0 and f(S=0) == 0                     # empty: a successful no-op
    assert fwd(None, None, None, None, None, B=0) == 0 and bwd(ptrs=[None] * 9, ws=None, B=2, S=0) == 0
    assert fwd(D=32, B=0) == E_SHAPE                            # the shape is checked even when there is nothing to do
    assert fwd(q=a + 2) == E_ALIGN and bwd(ptrs=[a] * 8 + [a + 8]) == E_ALIGN
    need = wsb(1, 8, 2, 2, 64)
    assert bwd(nws=need - 1) == E_WSPACE and bwd(nws=0) == E_WSPACE
    assert b"workspace" in lib.onebit_last_error()
    # the workspace: positive, non-decreasing in S, and at least the fp32 delta [B, H, S]
    sizes = [wsb(2, S, 4, 2, 128) for S in (1, 2, 63, 64, 65, 1000, 2048, 2049, 1 << 20)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[-2] > sizes[0]
    assert all(s >= 2 * 4 * S * 4 for s, S in zip(sizes, (1, 2, 63, 64, 65, 1000, 2048, 2049, 1 << 20)))
    assert wsb(0, 0, 0, 0, 0) > 0


def test_cpu_tensors_and_fp32_on_the_hip_route_raise():
    from onebit_amd.train_model import OneBitLlamaForCausalLMTrain, flash_attention_train
    q = torch.zeros(1, 4, 2, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        flash_attention_train(q, q, q)
    cfg = OneBitLlamaConfig(**M.CONFIGS["mha"])
    with pytest.raises(RuntimeError, match="float16 only"):
        OneBitLlamaForCausalLMTrain(cfg, dtype=torch.float32, attention="hip")
    with pytest.raises(ValueError):
        OneBitLlamaForCausalLMTrain(cfg, attention="sdpa")
    assert OneBitLlamaForCausalLMTrain(cfg, dtype=torch.float32).attention == "eager"
    model = OneBitLlamaForCausalLMTrain(cfg, dtype=torch.float16)
    assert model.attention == "hip"
    model.load_state_dict({k: v.half() for k, v in M.make_params(M.CONFIGS["mha"], 1).items()}, strict=True)
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="GPU"):
        model(ids)
    with pytest.raises(NotImplementedError, match="attention weights"):
        model(ids, output_attentions=True)
    with pytest.raises(NotImplementedError) as e1:
        from onebit_amd.kd import KDLoss
        KDLoss(kd_gamma=0.1)
    with pytest.raises(NotImplementedError) as e2:
        model(ids, output_attentions=True)
    assert str(e1.value) == str(e2.value)
