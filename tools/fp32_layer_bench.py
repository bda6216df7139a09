"""Time the fp32 route of the 1-bit linear layer (onebit_amd/csrc/ob_f32.h) on one GPU.

Per shape, one whole layer call (GEMM or GEMV + LayerNorm):
  fp32          BitLinearInf with fp32 parameters (the new route; the query's answer is printed)
  fp16          the fp16 module call at the same shape
  fp32 generic  the generic fp32 kernels, reached through the C ABI with the packed rows at pitch K / 8 + 1

Device-side timing (events around a window of calls on one stream), every shape warmed up, windows sized to ~0.2 s and
repeated; best and median window are printed.  FLOP = 2 T K N (the LayerNorm's are not counted, its time is).

    python tools/fp32_layer_bench.py [--out FILE] [--quick] [--no-generic]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2048, 4096, 11008), (2048, 11008, 4096), (512, 4096, 4096), (1, 4096, 11008), (1, 11008, 4096)]
F32 = 1


def time_calls(fn, target_s, min_iters, repeats):
    """[seconds per call] of `repeats` windows; each window is sized from a first timed call to last ~target_s"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    one = max(a.elapsed_time(b) * 1e-3, 1e-7)
    iters = max(min_iters, min(20000, int(target_s / one)))
    out = []
    for _ in range(repeats):
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / iters)
    return out, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="short windows (for a profiler run)")
    ap.add_argument("--no-generic", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp32_layer_bench: no GPU visible (timings are taken on the device; there is no fallback)")
    from onebit_amd import BitLinearInf, _lib
    from onebit_amd.bitnet import _stream_ptr
    lib = _lib.load()
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(0)
    try:
        clock = f"{torch.cuda.clock_rate(0)} MHz before the first launch (idle)"
    except Exception as e:                                     # (needs the SMI python binding)
        clock = f"not readable here ({type(e).__name__})"
    lines = [f"device {prop.name}  CUs {prop.multi_processor_count}  engine clock {clock}  torch {torch.__version__}  "
             f"(clocks as the machine sets them: nothing pinned)"]
    target, reps = (0.02, 2) if args.quick else (0.2, 5)
    g = torch.Generator(device="cpu").manual_seed(0)
    for T, K, N in SHAPES:
        packed = torch.randint(0, 256, (N, K // 8), generator=g, dtype=torch.uint8).view(torch.int8).to(dev)
        h = (0.5 + torch.rand(K, generator=g)).to(dev)
        gs = (0.5 + torch.rand(N, generator=g)).to(dev)
        x = torch.randn(T, K, generator=g).to(dev)
        res = {}
        for name, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
            m = BitLinearInf(K, N, dtype=dt).to(dev)
            m.weight.data, m.input_factor.data, m.weight_scale.data = packed, h.to(dt), gs.to(dt)
            xd = x.to(dt)
            with torch.no_grad():
                res[name] = time_calls(lambda: m(xd), target, 5, reps)
        if not args.no_generic:
            odd = torch.zeros(N, K // 8 + 1, dtype=torch.int8, device=dev)
            odd[:, :K // 8] = packed
            assert lib.onebit_linear_f32_route(T, K, N, odd.stride(0)) == 0
            y = torch.empty(T, N, dtype=torch.float32, device=dev)

            def generic():
                rc = lib.onebit_linear_forward(odd.data_ptr(), odd.stride(0), x.data_ptr(), h.data_ptr(), gs.data_ptr(), None, y.data_ptr(), None,
                                               None, 0, T, K, N, F32, 1e-5, 0, _stream_ptr(dev))
                assert rc == 0, rc
            res["fp32 generic"] = time_calls(generic, target / 4, 2, 2)
        route = lib.onebit_linear_f32_route(T, K, N, K // 8)
        lines.append(f"[{T}, {K}] -> {N}   (onebit_linear_f32_route = {route}; packed bytes {N * K // 8 / 1e6:.2f} MB)")
        for name, (ts, iters) in res.items():
            best, med = min(ts), statistics.median(ts)
            lines.append(f"    {name:<13s} best {best * 1e6:10.1f} us   median {med * 1e6:10.1f} us   {2.0 * T * K * N / best / 1e12:8.2f} TFLOP/s   "
                         f"{N * K / 8 / best / 1e9:8.1f} GB/s of packed rows   ({len(ts)} windows of {iters} calls)")
        if "fp32 generic" in res:
            lines.append(f"    fp32 route vs generic kernel: {min(res['fp32 generic'][0]) / min(res['fp32'][0]):.1f} x;  vs the fp16 call: "
                         f"{min(res['fp32'][0]) / min(res['fp16'][0]):.2f} x its time")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
