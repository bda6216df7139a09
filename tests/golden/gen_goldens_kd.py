#!/usr/bin/env python3
"""Generate tests/golden/kd_loss.npz from the REAL reference's knowledge-distillation objective.

Runs only in the build container, on the CPU, where /root/reference exists (nothing at test / bench time reads it).
``llama_factory/llamafactory/kd.py`` imports a trainer stack that is not needed for the loss, so only the AST nodes of
``KDTrainer.ce_loss`` and ``KDTrainer.compute_loss`` are compiled and executed here, in memory (the technique of
gen_goldens.py for the packer); no reference source text is written anywhere.  The two functions are called with stub
model objects that return canned logits and hidden states and, as the student model does, the causal-LM cross-entropy of
its own logits; the result is differentiated in float64.

Output is data only:  kd_loss.npz  B=2, S=5, V=320, H=64, 3 layers (4 hidden states per model), labels with some -100:
  s_logits, t_logits, labels, s_h{i}, t_h{i}              the inputs (fp32 values)
  case{c}_alpha / _beta / _scale                          c = 0: alpha 0.8, beta 1, scale 0.01;  c = 1: the scripts' alpha 1.0
  case{c}_loss, case{c}_kl                                compute_loss's value and ce_loss's (float64)
  case{c}_g_logits, case{c}_g_h{i} (i < 3)                gradients w.r.t. the student's logits and hidden states (float64);
                                                          the LAST hidden state gets none (the loop runs over n_layers entries)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_goldens_kd.py
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
B, S, V, H, LAYERS = 2, 5, 320, 64, 3


def load_ref_kd():
    path = f"{REF}/llama_factory/llamafactory/kd.py"
    tree = ast.parse(open(path).read(), filename=path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "KDTrainer"]
    assert len(cls) == 1
    fns = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name in ("ce_loss", "compute_loss")]
    assert [f.name for f in fns] == ["ce_loss", "compute_loss"]
    ns = {"torch": torch, "F": F, "logger": types.SimpleNamespace(info=lambda *a, **k: None)}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns["ce_loss"], ns["compute_loss"]


class _Model:
    """What compute_loss touches of the wrapped student: the KD hyper-parameters, .model.layers, .teacher_model, __call__."""

    def __init__(self, s_logits, s_states, t_logits, t_states, alpha, beta, scale):
        self.kd_alpha, self.kd_beta, self.kd_gamma, self.kd_loss_scale = alpha, beta, 0.0, scale
        self.model = types.SimpleNamespace(layers=[None] * LAYERS)
        self._s, self._sh, self._t, self._th = s_logits, s_states, t_logits, t_states

    def teacher_model(self, labels=None, output_hidden_states=False, output_attentions=False):
        assert not output_attentions
        return types.SimpleNamespace(logits=self._t, hidden_states=self._th if output_hidden_states else None, attentions=None)

    def __call__(self, labels=None, output_hidden_states=False, output_attentions=False):
        assert not output_attentions
        # the causal-LM loss of the student's own logits (position s against labels[:, s + 1], mean over labelled rows)
        loss = F.cross_entropy(self._s[:, :-1, :].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100)
        return types.SimpleNamespace(loss=loss, logits=self._s, hidden_states=self._sh if output_hidden_states else None,
                                     attentions=None)


def main():
    ce_loss, compute_loss = load_ref_kd()
    trainer = types.SimpleNamespace()
    trainer.ce_loss = lambda s, t: ce_loss(trainer, s, t)
    g = torch.Generator().manual_seed(2024)
    out = {
        "s_logits": (2.0 * torch.randn(B, S, V, generator=g)).numpy(),
        "t_logits": (2.0 * torch.randn(B, S, V, generator=g)).numpy(),
    }
    labels = torch.randint(0, V, (B, S), generator=g)
    labels[0, :2] = -100
    labels[1, 3] = -100
    out["labels"] = labels.numpy()
    for i in range(LAYERS + 1):
        out[f"s_h{i}"] = torch.randn(B, S, H, generator=g).numpy()
        out[f"t_h{i}"] = (out[f"s_h{i}"] + 0.5 * torch.randn(B, S, H, generator=g).numpy()).astype(np.float32)
    for c, (alpha, beta, scale) in enumerate([(0.8, 1.0, 0.01), (1.0, 1.0, 0.01)]):
        s = torch.from_numpy(out["s_logits"]).double().requires_grad_(True)
        t = torch.from_numpy(out["t_logits"]).double()
        sh = tuple(torch.from_numpy(out[f"s_h{i}"]).double().requires_grad_(True) for i in range(LAYERS + 1))
        th = tuple(torch.from_numpy(out[f"t_h{i}"]).double() for i in range(LAYERS + 1))
        model = _Model(s, sh, t, th, alpha, beta, scale)
        loss = compute_loss(trainer, model, {"labels": labels})
        loss.backward()
        assert sh[LAYERS].grad is None and all(h.grad is not None for h in sh[:LAYERS])
        out[f"case{c}_alpha"], out[f"case{c}_beta"], out[f"case{c}_scale"] = np.float64(alpha), np.float64(beta), np.float64(scale)
        out[f"case{c}_loss"] = loss.detach().numpy()
        out[f"case{c}_kl"] = trainer.ce_loss(s.detach(), t).numpy()
        out[f"case{c}_g_logits"] = s.grad.numpy()
        for i in range(LAYERS):
            out[f"case{c}_g_h{i}"] = sh[i].grad.numpy()
        print(f"case {c}: loss {float(loss.detach()):.12f} kl {float(out[f'case{c}_kl']):.12f}")
    np.savez_compressed(f"{OUT}/kd_loss.npz", **out)
    print("kd_loss.npz bytes:", os.path.getsize(f"{OUT}/kd_loss.npz"))


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("reference not present; fixtures can only be regenerated in the build container")
    torch.manual_seed(0)
    torch.set_num_threads(4)
    main()
