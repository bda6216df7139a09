#!/usr/bin/env python3
"""Forward + backward time of ``flash_attention_train`` against torch's fused attention on the training shape.

Both sides get the model's tensors: token-major ``q [B, S, H, D]`` and ``k, v [B, S, Hkv, D]`` with a gradient ``dO [B, S, H, D]``.
``flash_attention_train`` consumes them as they are.  ``torch.nn.functional.scaled_dot_product_attention(is_causal=True)`` wants
``[B, H, S, D]``; the transposes this layout forces (views on the way in, one contiguous copy of the output on the way out, and their
backward) are inside its timed region, as they would be inside a model.

Shapes: the reference's training shape (scripts/llama_7b.sh: 4 sequences of 2048 per device, 32 heads of 128) and the 13B head
count (40).  Timing: device events around ``--iters`` forward + backward pairs after ``--warmup`` pairs, the two sides alternating
in ``--rounds`` rounds so that drift hits both; the median round is reported with the spread.  "Useful" FLOP/s counts the causal half
of seven ``S x S x D`` products -- two forward, five backward, the usual convention for either side -- at 2 flops per multiply-add:
``7 * 2 * B * H * (S^2 / 2) * D``; the recomputation this build's backward does on top (nine products, not five) is not counted.

Writes profiles/train_attention.txt (or under the directory OB_PROFILES_DIR names).  Needs the GPU: there is no fallback.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [("7B", 4, 2048, 32, 32, 128), ("13B", 4, 2048, 40, 40, 128)]


def useful_flops(B, S, H, D):
    """causal: half of the S x S pairs; 2 flops per multiply-add; 2 products forward, 5 backward"""
    return 7 * 2 * B * H * (S * S / 2) * D


def hip_pair(q, k, v, d_o):
    from onebit_amd.train_model import flash_attention_train
    o = flash_attention_train(q, k, v)
    o.backward(d_o)
    return o


def sdpa_pair(q, k, v, d_o):
    kw = {"enable_gqa": True} if q.shape[2] != k.shape[2] else {}
    o = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True, **kw)
    o = o.transpose(1, 2).contiguous()
    o.backward(d_o)
    return o


def time_ms(fn, args, warmup, iters):
    q, k, v, _ = args
    for _ in range(warmup):
        fn(*args)
        q.grad = k.grad = v.grad = None
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn(*args)
        q.grad = k.grad = v.grad = None
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("train_attention_bench: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    out_dir = os.environ.get("OB_PROFILES_DIR") or os.path.join(ROOT, "profiles")
    out = a.out or os.path.join(out_dir, "train_attention.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lines = [f"# tools/train_attention_bench.py  device {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# forward + backward per call, ms; median of {a.rounds} alternating rounds of {a.iters} calls after {a.warmup} warm-up calls"]
    for name, B, S, H, Hkv, D in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        q, k, v = (torch.randn(B, S, h, D, device=dev, dtype=torch.float16, generator=g).requires_grad_(True) for h in (H, Hkv, Hkv))
        d_o = torch.randn(B, S, H, D, device=dev, dtype=torch.float16, generator=g)
        args = (q, k, v, d_o)
        # same function, to fp16 round-off, on the inputs that are timed
        o_h, o_s = hip_pair(*args), None
        gh = [t.grad.clone() for t in (q, k, v)]
        q.grad = k.grad = v.grad = None
        o_s = sdpa_pair(*args)
        gs = [t.grad.clone() for t in (q, k, v)]
        q.grad = k.grad = v.grad = None
        rel = lambda x, y: float((x.float() - y.float()).norm() / y.float().norm())
        agree = [rel(o_h, o_s)] + [rel(x, y) for x, y in zip(gh, gs)]
        hip, sdpa = [], []
        for _ in range(a.rounds):
            hip.append(time_ms(hip_pair, args, a.warmup, a.iters))
            sdpa.append(time_ms(sdpa_pair, args, a.warmup, a.iters))
        mh, ms = statistics.median(hip), statistics.median(sdpa)
        fl = useful_flops(B, S, H, D)
        lines += [f"{name}  B={B} S={S} H={H} Hkv={Hkv} D={D}",
                  f"  flash_attention_train   {mh:8.3f} ms  (min {min(hip):.3f} max {max(hip):.3f})  {fl / mh / 1e9:7.1f} useful TFLOP/s",
                  f"  sdpa + transposes       {ms:8.3f} ms  (min {min(sdpa):.3f} max {max(sdpa):.3f})  {fl / ms / 1e9:7.1f} useful TFLOP/s",
                  f"  ratio flash_attention_train / sdpa  {mh / ms:.2f}x the time",
                  "  rel-L2 between the two (o, dq, dk, dv): " + " ".join(f"{x:.1e}" for x in agree)]
        del q, k, v, d_o, args, o_h, o_s, gh, gs
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
