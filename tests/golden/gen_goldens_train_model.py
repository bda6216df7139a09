#!/usr/bin/env python3
"""Train-mode model fixture from the REAL reference model (build container only).

Imports the reference's forked transformers (read-only, PYTHONDONTWRITEBYTECODE=1) with the two over-strict dependency pins
shimmed, builds a tiny ``BitLlamaForCausalLM`` in float32 on the CPU for each record of
``tests/_train_model_ref.py`` (``mha``, and ``gqa`` with one kv head), loads the seeded parameters of ``make_params`` into it,
and records one forward with labels and one backward of its loss: input_ids, labels, logits, every hidden state, the loss, the
gradients of ``GRAD_KEYS`` (the embedding and lm_head are frozen in the reference; they are unfrozen for the recording), and the
model's state-dict keys with their shapes.  The parameters themselves are not stored (1.6 MB): the seed regenerates them.
Output: tests/golden/train_model_tiny.npz (data only).

Usage (from the repo root, REF = the reference checkout's transformers/src):
  PYTHONDONTWRITEBYTECODE=1 ONEBIT_REFERENCE_SRC=$REF python tests/golden/gen_goldens_train_model.py
"""
import importlib.metadata as md
import os
import sys

import numpy as np
import torch

_orig = md.version
_fake = {"tokenizers": "0.14.1", "huggingface-hub": "0.17.3", "huggingface_hub": "0.17.3"}
md.version = lambda n: _fake.get(n, _orig(n))

REF_SRC = os.environ.get("ONEBIT_REFERENCE_SRC", "")
if not os.path.isdir(REF_SRC):
    sys.exit("set ONEBIT_REFERENCE_SRC to the reference's transformers/src; the fixture can only be regenerated where it is present")
sys.path.insert(0, REF_SRC)
from transformers import BitLlamaConfig, BitLlamaForCausalLM  # noqa: E402  (the reference fork)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _train_model_ref as R  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_model_tiny.npz")


def record(name):
    cfg = R.CONFIGS[name]
    sd = R.make_params(cfg, R.SEEDS[name])
    ids, labels = R.make_batch(cfg, R.SEEDS[name])
    model = BitLlamaForCausalLM(BitLlamaConfig(**cfg)).to(torch.float32)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in m or "inv_freq" in m for m in missing), (missing, unexpected)
    model.train()
    params = dict(model.named_parameters())
    for k in ("model.embed_tokens.weight", "lm_head.weight"):
        params[k].requires_grad_(True)
    o = model(ids, labels=labels, output_hidden_states=True, use_cache=False)
    assert len(o.hidden_states) == cfg["num_hidden_layers"] + 1
    o.loss.backward()
    out = {"seed": np.array(R.SEEDS[name]), "input_ids": ids.numpy(), "labels": labels.numpy(),
           "logits": o.logits.detach().numpy(), "loss": o.loss.detach().numpy()}
    for i, h in enumerate(o.hidden_states):
        out[f"hidden_{i}"] = h.detach().numpy()
    for k in R.GRAD_KEYS:
        out["grad/" + k] = params[k].grad.numpy()
    keys = [k for k in model.state_dict() if "inv_freq" not in k]
    out["keys"] = np.array(keys)
    out["shapes"] = np.array([list(model.state_dict()[k].shape) + [0] * (2 - model.state_dict()[k].dim()) for k in keys], dtype=np.int64)
    out["trainable"] = np.array([k for k, p in params.items() if p.requires_grad and k not in ("model.embed_tokens.weight", "lm_head.weight")])
    for k, v in cfg.items():
        out["cfg_" + k] = np.array(v)
    print(name, "loss", float(o.loss), "logits rms", float(o.logits.pow(2).mean().sqrt()))
    return {f"{name}/{k}": v for k, v in out.items()}


if __name__ == "__main__":
    torch.set_num_threads(4)
    data = {}
    for n in R.RECORDS:
        data.update(record(n))
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT))
