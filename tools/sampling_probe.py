#!/usr/bin/env python3
"""Greedy vs sampled decode on the synthetic 7B model (top_k 50, top_p 0.9, temperature 0.8):
  - onebit_decode_step vs onebit_decode_step_sampled, one sequence at 128 and 1900 cached tokens (direct launches, the graph
    form the engine would replay has the same kernels)
  - the 32-slot batched step (keep_logits: the sampled form needs the logits) without and with the params rows
  - the standalone sampler (onebit_sample_rows) at B = 1 / 32 / 64, V = 32000
Alternating A/B windows, device events.  python tools/sampling_probe.py [--kernel-only]
(the sampler's kernel time: rocprofv3 --kernel-trace --stats -- python tools/sampling_probe.py --kernel-only)"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from onebit_amd import _lib
from onebit_amd.sampling import SamplingParams, pack, sample_logits

dev = torch.device("cuda:0")
SP = SamplingParams(temperature=0.8, top_k=50, top_p=0.9, seed=1234)


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def ab(fa, fb, n=64, rounds=5):
    for f in (fa, fb):
        window(f, 8)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, n))
        tb.append(window(fb, n))
    return sorted(ta)[rounds // 2], sorted(tb)[rounds // 2]


def kernel_only():
    V = 32000
    for B in (1, 32, 64):
        lg = (torch.randn(B, V, device=dev) * 3).half()
        pr = pack([SP] * B, dev)
        pos = torch.arange(B, dtype=torch.int32, device=dev)
        for _ in range(50):
            sample_logits(lg, pr, pos)
        torch.cuda.synchronize()
        print(f"sampler B={B} V={V}: {window(lambda: sample_logits(lg, pr, pos), 200) * 1e3:.1f} us per call (host launch included)", flush=True)


def main():
    if "--kernel-only" in sys.argv:
        kernel_only()
        return
    import bench
    from onebit_amd.engine import BatchedDecodeStep, DecodeEngine, fp16_view, step_variant
    from onebit_amd.llama import build_synthetic_model
    cfg = bench.model_config("7b")
    model = build_synthetic_model(cfg, seed=4242, device=dev)
    lib = _lib.load()
    eng = DecodeEngine(model, max_len=2048, use_graph=False)
    pr1 = pack([SP], dev)
    ids = torch.randint(0, cfg.vocab_size, (1, 16), generator=torch.Generator().manual_seed(3)).to(dev)
    eng.prime(ids)
    print("7B synthetic, top_k 50 / top_p 0.9 / temperature 0.8")
    for ctx in (128, 1900):
        key = step_variant(ctx, eng._long_from, eng._short_ok, eng._keyblock, eng._kb_chunk, eng._kb_top)
        st = eng._variants["short" if key == "64" else key]
        stream = lambda: torch.cuda.current_stream(dev).cuda_stream

        def greedy():
            eng.pos.fill_(ctx)
            _lib.check(lib.onebit_decode_step(ctypes.byref(eng._model), ctypes.byref(st), stream()), "decode")

        def sampled():
            eng.pos.fill_(ctx)
            _lib.check(lib.onebit_decode_step_sampled(ctypes.byref(eng._model), ctypes.byref(st), pr1.data_ptr(), stream()), "decode_sampled")
        a, b = ab(greedy, sampled)
        print(f"decode step at {ctx} cached tokens: greedy {a:.4f} ms/token, sampled {b:.4f} ms/token ({b / a:.3f}x)", flush=True)
    del eng
    B, L = 32, 512
    cache = fp16_view(model).new_cache(B, L)
    step = BatchedDecodeStep(model, cache.layers, B, L, keep_logits=True)
    step.tokens.copy_(torch.randint(0, cfg.vocab_size, (B,), generator=torch.Generator().manual_seed(5)).int())
    prB = pack([SP.with_stream(b) for b in range(B)], dev)

    def bg():
        step.pos.fill_(128)
        step.launch()

    def bs():
        step.pos.fill_(128)
        step.launch(params=prB)
    a, b = ab(bg, bs, n=32)
    print(f"32-slot batched step at 128 cached tokens: greedy {a:.4f} ms/step, sampled {b:.4f} ms/step ({b / a:.3f}x)", flush=True)
    kernel_only()


if __name__ == "__main__":
    main()
