#!/usr/bin/env python3
"""Time the SVID kernels (onebit_amd/svid.py, csrc/ob_svid.h) against the torch op sequence on the same device, in the same
run, at the projection shapes of LLaMA-7B / 13B: one alternating iteration on both routes and the emit pass.

Per shape, dtype and path: time per call (device events around `iters` calls after a warm-up) and N K sizeof(A) bytes -- one
read of A, what the one-pass iteration and the emit pass need -- over that time in GB/s.  The torch sequence:
`A.abs() @ h`, `A.abs().T @ w` (an iteration's two products) and `torch.sign(A) * 0.01`, `pack_signs(A)` (the emit pass).
The JSON rows are printed and appended to profiles/svid.txt (or to --out).

  python tools/svid_bench.py [--iters 10] [--warmup 3] [--small] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from onebit_amd import pack_signs  # noqa: E402
from onebit_amd.svid import SvidWork, svid_init  # noqa: E402

DEV = "cuda:0"
SHAPES = [(4096, 11008), (11008, 4096), (13824, 5120)]


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="one eighth of the rows (a quick check of the tool itself)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svid.txt"), help="append the JSON rows to this file")
    args = ap.parse_args()
    rows = []
    for N, K in SHAPES:
        if args.small:
            N //= 8
        for dt in (torch.float16, torch.float32):
            g = torch.Generator(device=DEV).manual_seed(0)
            a = (0.02 * torch.randn(N, K, generator=g, device=DEV)).to(dt)
            nbytes = N * K * a.element_size()
            w0, h0 = svid_init(N, K, float(a.float().abs().mean()), "float32")
            w, h = torch.from_numpy(w0).to(DEV), torch.from_numpy(h0).to(DEV)
            wk = SvidWork(a, N, K)
            latent = torch.empty((N, K), dtype=dt, device=DEV)
            packed = torch.empty((N, K // 8), dtype=torch.int8, device=DEV)
            wt, ht = w.to(dt), h.to(dt)
            wi, hi = w.clone(), h.clone()           # iterated in place: the values move towards the fit, the work per call does not
            paths = {
                "iterate one-pass": lambda: wk.iterate(wi, hi, 1),
                "iterate two-pass": lambda: wk.iterate(wi, hi, 2),
                "iterate torch": lambda: (a.abs() @ ht, a.abs().T @ wt),
                "emit latent+packed+sums": lambda: wk.emit(w, h, latent=latent, packed=packed),
                "emit packed only": lambda: wk.emit(w, h, packed=packed, sums=False),
                "emit torch": lambda: (torch.sign(a) * 0.01, pack_signs(a)),
            }
            for name, fn in paths.items():
                ms = _time(fn, args.warmup, args.iters)
                row = {"shape": [N, K], "dtype": str(dt).replace("torch.", ""), "path": name, "ms": round(ms, 4),
                       "GBps_over_one_read_of_A": round(nbytes / (ms * 1e-3) / 1e9, 1)}
                print(json.dumps(row), flush=True)
                rows.append(row)
            del a, wk, latent, packed
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
