#!/usr/bin/env python3
"""Time the fused knowledge-distillation loss (onebit_amd/kd.py, csrc/ob_kd.h) against the torch op sequence of the
restatement (tests/_kd_ref.py) on the same device, in the same run, at the reference's training shape
(scripts/llama_7b.sh: per-device batch 4, cutoff 2048, vocabulary 32000; 32 hidden-state pairs of [8192, 4096]).

Per shape and path: forward and forward + backward time (device events around `iters` calls after a warm-up), the
algorithmic bytes over that time as a share of the 8 TB/s HBM peak (forward 2 T W e, backward 3 T W e: each operand read
once, the gradient written once), and the peak allocated memory above the inputs.  Results: profiles/kd_loss.txt.

  python tools/kd_loss_bench.py [--iters 10] [--warmup 3] [--small] [--only fused|torch]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _kd_ref  # noqa: E402
from onebit_amd.kd import kd_hidden_loss, kd_token_loss  # noqa: E402

DEV = "cuda:0"
PEAK = 8.0e12


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


def _measure(name, path, fwd, fwd_bwd, bytes_fwd, bytes_bwd, args):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fwd_bwd()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    t_f = _time(fwd, args.warmup, args.iters)
    t_fb = _time(fwd_bwd, args.warmup, args.iters)
    row = {"shape": name, "path": path, "fwd_ms": round(t_f, 4), "fwd_bwd_ms": round(t_fb, 4),
           "fwd_frac_of_8TBs": round(bytes_fwd / (t_f * 1e-3) / PEAK, 4),
           "fwd_bwd_frac_of_8TBs": round((bytes_fwd + bytes_bwd) / (t_fb * 1e-3) / PEAK, 4),
           "peak_extra_MB": round(peak / 2 ** 20, 1)}
    print(json.dumps(row), flush=True)
    return row


def token_shape(B, S, V, dtype, args):
    g = torch.Generator(device=DEV).manual_seed(0)
    s = (2 * torch.randn(B, S, V, device=DEV, generator=g)).to(dtype).requires_grad_(True)
    t = (2 * torch.randn(B, S, V, device=DEV, generator=g)).to(dtype)
    labels = torch.randint(0, V, (B, S), device=DEV, generator=g)
    e = s.element_size()
    name = f"token [{B},{S},{V}] {str(dtype).split('.')[-1]}"
    nbytes = B * S * V * e

    def fused_f():
        return kd_token_loss(s, t, labels, kd_alpha=0.8, kd_loss_scale=1.0)[0]

    def torch_f():
        return _kd_ref.token_loss(s, t, labels, 0.8, 1.0)[0]

    def fb(f):
        def run():
            s.grad = None
            f().backward()
        return run

    rows = []
    if args.only != "torch":
        rows.append(_measure(name, "fused", fused_f, fb(fused_f), 2 * nbytes, 3 * nbytes, args))
    if args.only != "fused":
        rows.append(_measure(name, "torch", torch_f, fb(torch_f), 2 * nbytes, 3 * nbytes, args))
    return rows


def hidden_shape(pairs, T, H, dtype, args):
    g = torch.Generator(device=DEV).manual_seed(1)
    ss = [torch.randn(T, H, device=DEV, generator=g).to(dtype).requires_grad_(True) for _ in range(pairs)]
    ts = [torch.randn(T, H, device=DEV, generator=g).to(dtype) for _ in range(pairs)]
    name = f"hidden {pairs} x [{T},{H}] {str(dtype).split('.')[-1]}"
    nbytes = pairs * T * H * ss[0].element_size()

    def fused_f():
        return kd_hidden_loss(ss, ts)

    def torch_f():
        return _kd_ref.hidden_loss(ss, ts)

    def fb(f):
        def run():
            for x in ss:
                x.grad = None
            f().backward()
        return run

    rows = []
    if args.only != "torch":
        rows.append(_measure(name, "fused", fused_f, fb(fused_f), 2 * nbytes, 3 * nbytes, args))
    if args.only != "fused":
        rows.append(_measure(name, "torch", torch_f, fb(torch_f), 2 * nbytes, 3 * nbytes, args))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a sixteenth of the rows (a quick look, not a result)")
    ap.add_argument("--only", choices=["fused", "torch"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kd_loss_bench needs a GPU: a CPU run says nothing about these kernels")
    S = 128 if args.small else 2048
    rows = []
    rows += token_shape(4, S, 32000, torch.float32, args)
    rows += token_shape(4, S, 32000, torch.float16, args)
    rows += hidden_shape(32, 4 * S, 4096, torch.float16, args)
    by = {(r["shape"], r["path"]): r for r in rows}
    for shape in dict.fromkeys(r["shape"] for r in rows):
        f, t = by.get((shape, "fused")), by.get((shape, "torch"))
        if f and t:
            print(json.dumps({"shape": shape, "speedup_fwd": round(t["fwd_ms"] / f["fwd_ms"], 2),
                              "speedup_fwd_bwd": round(t["fwd_bwd_ms"] / f["fwd_bwd_ms"], 2),
                              "peak_memory_ratio": round(f["peak_extra_MB"] / max(t["peak_extra_MB"], 1e-9), 3)}), flush=True)


if __name__ == "__main__":
    main()
