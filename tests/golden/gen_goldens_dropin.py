"""Records the drop-in contract of the reference's ``BitLlamaForCausalLMInf`` (modeling_bitllama.py:1512-1611) into
dropin_contract.json, the fixture of tests/test_dropin_reference_cpu.py:
  * every ``BitLinearInf(...)`` construction the reference model makes (module name, positional and keyword
    arguments), recorded with the reference's import of ``BitLinearInf`` (modeling_bitllama.py:25) monkey-patched to
    ``onebit_amd.BitLinearInf`` as INTEGRATION.md section 1 documents;
  * the state-dict contract (keys in order, shapes, dtypes) of the unpatched reference model, which the patched one
    must equal (checked here before anything is written).
Needs the reference fork's ``transformers/src``; usage:
  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_goldens_dropin.py <reference>/transformers/src"""
import importlib.metadata as md
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_contract.json")

# the model shape of tests/test_dropin_reference_cpu.py
KW = dict(vocab_size=320, hidden_size=256, intermediate_size=688, num_hidden_layers=2, num_attention_heads=4,
          max_position_embeddings=64)


def contract(model):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()]


def main(ref_src):
    orig = md.version
    fake = {"tokenizers": "0.14.1", "huggingface-hub": "0.17.3", "huggingface_hub": "0.17.3"}
    md.version = lambda n: fake.get(n, orig(n))
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref_src)
    import transformers.models.bitnet as ref_bitnet
    import transformers.models.bitllama.modeling_bitllama as mb
    from transformers import BitLlamaConfig

    import onebit_amd
    ref_cls = mb.BitLinearInf
    assert ref_cls is ref_bitnet.BitLinearInf
    out = {"config": KW, "cases": {}}
    for attention_bias in (False, True):
        cfg = BitLlamaConfig(attention_bias=attention_bias, **KW)
        torch.manual_seed(0)
        ref_model = mb.BitLlamaForCausalLMInf(cfg)
        calls = []

        def recording(*args, **kwargs):
            m = onebit_amd.BitLinearInf(*args, **kwargs)
            calls.append((m, list(args), dict(kwargs)))
            return m
        try:
            ref_bitnet.BitLinearInf = mb.BitLinearInf = recording
            model = mb.BitLlamaForCausalLMInf(cfg)
        finally:
            ref_bitnet.BitLinearInf = mb.BitLinearInf = ref_cls
        names = {id(m): n for n, m in model.named_modules()}
        assert not any(isinstance(m, ref_cls) for m in model.modules())
        assert len(calls) == sum(isinstance(m, ref_cls) for m in ref_model.modules()) == 7 * KW["num_hidden_layers"]
        assert contract(model) == contract(ref_model)
        out["cases"][str(attention_bias).lower()] = {
            "bitlinear_calls": [{"name": names[id(m)], "args": a, "kwargs": k} for m, a, k in calls],
            "state_dict": contract(ref_model),
        }
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main(sys.argv[1])
