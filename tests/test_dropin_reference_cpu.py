"""Drop-in boundary inside the REFERENCE's own model class (SURVEY.md section 8 row b):
``BitLlamaForCausalLMInf`` (modeling_bitllama.py:1512-1611) built around ``onebit_amd.BitLinearInf`` by the documented
monkey-patch of the import at modeling_bitllama.py:25 -- the seven call sites per layer (:229-231, :451-454) then
construct THIS repo's module.  The reference's side is recorded in golden/dropin_contract.json (gen_goldens_dropin.py):
the arguments of every one of those constructions and the unpatched reference model's state dict (keys in order, shapes,
dtypes).  Checked: each recorded call builds this repo's module with the recorded parameters, module count, this repo's
model has the reference's state-dict contract, a reference state dict loads cleanly, ``.half()`` leaves ``weight`` int8
and casts only the floating parameters (modeling_utils.py:696 semantics), the converter's in-place ``.data`` assignments
(convert_llama_to_infer_ckpt.py:32-34) take, and forward on CPU tensors refuses loudly (no CPU fallback)."""
import json
import os

import pytest
import torch


@pytest.fixture(scope="module")
def contract(golden_dir):
    with open(os.path.join(golden_dir, "dropin_contract.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("attention_bias", [False, True])
def test_reference_model_built_around_our_module(contract, attention_bias):
    import onebit_amd
    from onebit_amd.llama import OneBitLlamaConfig, OneBitLlamaForCausalLM
    KW = contract["config"]
    case = contract["cases"][str(attention_bias).lower()]
    ref_sd = {k: (tuple(shape), getattr(torch, dt)) for k, shape, dt in case["state_dict"]}
    # the reference's call sites, replayed: each builds this repo's module with the parameters the reference checkpoint holds
    calls = case["bitlinear_calls"]
    assert len(calls) == 7 * KW["num_hidden_layers"]
    for c in calls:
        m = onebit_amd.BitLinearInf(*c["args"], **c["kwargs"])
        for n, p in m.named_parameters():
            assert (tuple(p.shape), p.dtype) == ref_sd[c["name"] + "." + n], (c["name"], n)
        assert {c["name"] + "." + n for n, _ in m.named_parameters()} == {k for k in ref_sd if k.rsplit(".", 1)[0] == c["name"]}
    cfg = OneBitLlamaConfig(attention_bias=attention_bias, **KW)
    torch.manual_seed(0)
    model = OneBitLlamaForCausalLM(cfg, dtype=torch.float32)
    ours = [m for m in model.modules() if isinstance(m, onebit_amd.BitLinearInf)]
    assert len(ours) == len(calls)
    assert [n for n, m in model.named_modules() if isinstance(m, onebit_amd.BitLinearInf)] == [c["name"] for c in calls]
    # identical state-dict contract
    sd = model.state_dict()
    assert list(sd) == list(ref_sd)
    for k in sd:
        assert (tuple(sd[k].shape), sd[k].dtype) == ref_sd[k], k
    # a (random) reference checkpoint loads by key
    g = torch.Generator().manual_seed(1)
    sd_ref = {}
    for k, (shape, dt) in ref_sd.items():
        if dt == torch.int8:
            sd_ref[k] = torch.randint(-128, 128, shape, generator=g, dtype=torch.int8)
        else:
            sd_ref[k] = (torch.randn(shape, generator=g) * 0.1).to(dt)
    missing, unexpected = model.load_state_dict(sd_ref, strict=True)
    assert not missing and not unexpected
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd_ref[k]), k
    for m in ours:
        assert all(not p.requires_grad for p in m.parameters())
        assert (m.bias is not None) == (attention_bias and m.out_features in (KW["hidden_size"],) and m in
                                       [x for l in model.model.layers for x in (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.o_proj)])
    # .half(): floating parameters cast, packed weight stays int8 (modeling_utils.py:696 does the same at load)
    model.half()
    for m in ours:
        assert m.weight.dtype == torch.int8
        assert m.weight_scale.dtype == m.input_factor.dtype == torch.float16
        assert m.bias is None or m.bias.dtype == torch.float16
    # the converter's in-place assignments (convert_llama_to_infer_ckpt.py:32-34)
    m0 = ours[0]
    w_new = torch.randint(-128, 128, m0.weight.shape, generator=g, dtype=torch.int8)
    m0.weight.data = w_new
    m0.weight_scale.data = torch.ones_like(m0.weight_scale) * 0.5
    m0.input_factor.data = torch.ones_like(m0.input_factor) * 2.0
    assert torch.equal(model.state_dict()[next(k for k in sd if k.endswith("q_proj.weight"))], w_new)
    # no CPU fallback: the product path refuses CPU tensors instead of computing something else
    with pytest.raises((RuntimeError, ValueError)):
        model(torch.tensor([[1, 2, 3]]))
