#!/usr/bin/env python3
"""Generate tests/golden/sampling_warpers.npz from the REAL reference's logits warpers.

Runs only in the build container, where /root/reference exists (nothing at test time reads it).  Importing
``transformers`` from the reference tree fails on a tokenizers version check, so -- as gen_goldens.py does for the
packer -- only the AST nodes of ``TemperatureLogitsWarper``, ``TopKLogitsWarper`` and ``TopPLogitsWarper`` are compiled
and executed, in memory, with their docstring decorators dropped; no reference source text is written anywhere.

They are applied in ``_get_logits_warper`` order (temperature if != 1, top-k if != 0, top-p if < 1: generation/utils.py)
to seeded fp16 logits rows (fp32 scores, as generate() hands them over) without ties and without a cumulative mass near a
top-p boundary, so that the kept set is well defined.  Output (data only): the logits, the parameters and the kept masks.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_goldens_sampling.py
"""
import ast
import math
import os

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
CLASSES = ("TemperatureLogitsWarper", "TopKLogitsWarper", "TopPLogitsWarper")


def load_ref_warpers():
    path = f"{REF}/transformers/src/transformers/generation/logits_process.py"
    tree = ast.parse(open(path).read(), filename=path)
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
    assert len(nodes) == 3
    for cls in nodes:
        cls.bases = []
        for fn in cls.body:
            if isinstance(fn, ast.FunctionDef):
                fn.decorator_list = []
    ns = {"torch": torch, "math": math, "np": np}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return [ns[c] for c in CLASSES]


def main():
    Temp, TopK, TopP = load_ref_warpers()
    rng = np.random.default_rng(20261016)
    grid = [(t, k, p) for t in (0.6, 1.0, 1.5) for k in (0, 1, 5, 50) for p in (0.05, 0.5, 0.9, 1.0)]
    rng.shuffle(grid)
    vocabs = (50, 257, 1000)
    logits, params, masks, vs = [], [], [], []
    for j, (t, k, p) in enumerate(grid[:48]):
        V = vocabs[j % 3]
        while True:
            # tie-free rows: V distinct fp16 values of [-scale, scale]
            scale = rng.uniform(2.0, 8.0)
            pool = np.unique(np.linspace(-scale, scale, 20001).astype(np.float16))
            x = rng.choice(pool, V, replace=False).astype(np.float16)
            s = torch.from_numpy(x.astype(np.float32))[None]
            warpers = []
            if t != 1.0:
                warpers.append(Temp(t))
            if k != 0:
                warpers.append(TopK(top_k=k, min_tokens_to_keep=1))
            if p < 1.0:
                warpers.append(TopP(top_p=p, min_tokens_to_keep=1))
            for w in warpers:
                s = w(None, s)
            if p < 1.0:
                # no cumulative mass within 1e-4 of the top-p boundary (HF and the contract round it differently)
                sc = torch.from_numpy(x.astype(np.float32))[None] / t if t != 1.0 else torch.from_numpy(x.astype(np.float32))[None]
                if k:
                    sc = TopK(top_k=k)(None, sc)
                pr = torch.sort(sc.double().softmax(-1), descending=True)[0].cumsum(-1)
                if (pr - p).abs().min() < 1e-4:
                    continue
            break
        logits.append(np.pad(x, (0, 1000 - V)))
        params.append((t, k, p))
        masks.append(np.pad(torch.isfinite(s[0]).numpy(), (0, 1000 - V)))
        vs.append(V)
    np.savez_compressed(os.path.join(OUT, "sampling_warpers.npz"), logits=np.stack(logits), vocab=np.array(vs, dtype=np.int32),
                        temperature=np.array([q[0] for q in params], dtype=np.float32), top_k=np.array([q[1] for q in params], dtype=np.int32),
                        top_p=np.array([q[2] for q in params], dtype=np.float32), kept=np.stack(masks))
    print("wrote sampling_warpers.npz:", len(vs), "rows")


if __name__ == "__main__":
    main()
