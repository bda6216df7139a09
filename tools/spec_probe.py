"""Speculative decoding on the single-stream engine, measured on a synthetic 7B checkpoint (as bench.py builds it): what a
speculative step costs against the greedy step at the same context, what the multi-query attention saves, and the two bounds of
tokens/s (oracle drafts: every draft accepted; adversarial drafts: none).  Random weights make prompt-lookup ACCEPTANCE meaningless
as a quality figure, so none is reported: the break-even acceptance R(k) - 1 is what a real checkpoint has to beat.

    python tools/spec_probe.py [--out profiles/spec_decode.txt] [--rounds 5]

Every comparison alternates A / B inside one process on one device (warm-up first, medians over the rounds)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onebit_amd import _lib                                              # noqa: E402
from onebit_amd.engine import DecodeEngine, SpecStep                     # noqa: E402
from onebit_amd.llama import OneBitLlamaConfig, build_synthetic_model    # noqa: E402
from onebit_amd.speculative import SpecConfig                            # noqa: E402

DEV = torch.device("cuda:0")
KS = (1, 2, 4, 8)


def wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spec_decode.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cfg = OneBitLlamaConfig.llama_7b()
    model = build_synthetic_model(cfg, seed=1, device=DEV)
    max_len = 2048
    eng = DecodeEngine(model, max_len=max_len)
    for kc, vc in eng.cache.layers:
        kc.normal_()
        vc.normal_()
    g = torch.Generator().manual_seed(3)
    specs = {k: SpecStep(eng.model, eng.cache.layers, 1, max_len, SpecConfig(k), attn_chunk=eng._kb_chunk) for k in KS}
    say(f"# speculative decode step, synthetic 7B ({cfg.num_hidden_layers} layers), max_len {max_len}, attention chunk {eng._kb_chunk}; "
        f"{torch.cuda.get_device_name(0)}; medians of {args.rounds} alternating rounds")
    say("# ms per step: the speculative step WITH its 12-byte record read back every step (as generate runs it) | enqueued back to back, no read")
    NSTEP = 16
    for ctx in (128, 1900):
        hist = torch.randint(0, cfg.vocab_size, (ctx + 1,), generator=g).tolist()
        base, rd, nord = [], {k: [] for k in KS}, {k: [] for k in KS}
        snaps = {}
        for k, sp in specs.items():
            sp.arm(None)
            sp.seed(hist, 1 << 20)
            torch.cuda.synchronize()
            snaps[k] = (sp._ints.clone(), sp._host_pos)

        def run_base():
            eng.set_state(5, ctx)
            for _ in range(NSTEP):
                eng.step()

        def run_spec(k, read):
            sp = specs[k]
            sp._ints.copy_(snaps[k][0])
            sp._host_pos = snaps[k][1]
            sp.read_back = read
            ns = sp.splits(ctx + NSTEP * (k + 1) + k + 1)
            for _ in range(NSTEP):
                sp.step(ns=ns)
                if read:
                    sp.read_record()
            sp.read_back = True

        for r in range(args.rounds + 2):                                 # two warm-up rounds (the graphs are captured on the second use)
            tb = wall(run_base, NSTEP)
            tr = {k: wall(lambda k=k: run_spec(k, True), NSTEP) for k in KS}
            tn = {k: wall(lambda k=k: run_spec(k, False), NSTEP) for k in KS}
            if r >= 2:
                base.append(tb)
                for k in KS:
                    rd[k].append(tr[k])
                    nord[k].append(tn[k])
        b = statistics.median(base)
        say(f"context {ctx}: greedy DecodeEngine.step {b:.3f} ms/token ({1e3 / b:.0f} tok/s)")
        for k in KS:
            a, n = statistics.median(rd[k]), statistics.median(nord[k])
            say(f"  k = {k}: step {a:.3f} ms | {n:.3f} ms without the read ({a - n:+.3f} ms for the read-back);  R(k) = {a / b:.3f}: "
                f"break-even at {a / b - 1:.2f} accepted drafts per step; all {k} accepted: {(k + 1) * 1e3 / a:.0f} tok/s")
    # ---- the multi-query attention against k + 1 rows through the single-row kernel, 1900 cached tokens
    L, lib = _lib, _lib.load()
    H, D, chunk, ctx = cfg.num_attention_heads, cfg.head_dim, eng._kb_chunk, 1900
    nsplit = -(-max_len // chunk)
    kc, vc = eng.cache.layers[0]
    say(f"# attention alone at {ctx} cached tokens, {H} heads x {D}, chunk {chunk}, {nsplit} splits: Q rows of one sequence (50 launches per graph replay)")
    for Q in (5, 9):
        q = torch.randn(Q, H, D, device=DEV).half()
        o = torch.zeros(Q, H * D, dtype=torch.float16, device=DEV)
        rs = torch.zeros(Q, dtype=torch.int32, device=DEV)
        rp = torch.arange(ctx, ctx + Q, dtype=torch.int32, device=DEV)
        nb = int(lib.onebit_attention_decode_scratch_bytes(Q, H, nsplit))
        scr = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        sp = lambda: torch.cuda.current_stream(DEV).cuda_stream
        one = lambda: L.check(lib.onebit_attention_decode_rows(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), None, rs.data_ptr(), rp.data_ptr(),
                                                               Q, H, H, D, 1, max_len, chunk, nsplit, scr.data_ptr(), nb, sp()), "fdec")
        mq = lambda: L.check(lib.onebit_attention_decode_rows_mq(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), None, rs.data_ptr(), rp.data_ptr(),
                                                                 Q, Q, H, H, D, 1, max_len, chunk, nsplit, scr.data_ptr(), nb, sp()), "fdec_mq")
        graphs = []
        for fn in (one, mq):
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(50):
                    fn()
            graph.replay()
            graphs.append(graph)
        ta, tb = [], []
        for r in range(args.rounds + 1):
            for graph, acc in zip(graphs, (ta, tb)):
                t = wall(lambda: [graph.replay() for _ in range(4)], 200) * 1e3
                if r >= 1:
                    acc.append(t)
        a, b = statistics.median(ta), statistics.median(tb)
        say(f"  Q = {Q}: {Q} single-row workgroups per (head, split) {a:.2f} us | multi-query {b:.2f} us: time ratio {b / a:.2f} (K / V bytes: 1 / {Q})")
    # ---- tokens/s bounds through generate(): oracle drafts (a previous greedy run) and adversarial drafts
    S, n = 128, 256
    prompt = torch.randint(0, cfg.vocab_size, (1, S), generator=g).to(DEV)
    # the oracle is a previous greedy run THROUGH THE SAME STEP (no draft ever accepted): the GEMV step's tokens part from it at the
    # first near-tie of these random-weight logits, and drafts from another route stop being accepted there
    never = next(t for t in range(cfg.vocab_size) if t not in eng.generate(prompt, n)[0].tolist())
    ref = eng.generate(prompt, n, speculative=SpecConfig(1), drafts=lambda m: [never])[0].tolist()
    bad = next(t for t in range(cfg.vocab_size) if t not in ref)
    steps = {}
    res = {}
    for r in range(args.rounds + 1):
        t_prime = wall(lambda: eng.prime(prompt), 1)
        runs = [("greedy", lambda: eng.generate(prompt, n))]
        for k in KS:
            runs.append((f"oracle k={k}", lambda k=k: eng.generate(prompt, n, speculative=SpecConfig(k), drafts=lambda m: (ref[m:m + k] + [0] * k)[:k])))
            runs.append((f"adversarial k={k}", lambda k=k: eng.generate(prompt, n, speculative=SpecConfig(k), drafts=lambda m: [bad] * k)))
        runs.append(("prompt lookup k=4", lambda: eng.generate(prompt, n, speculative=SpecConfig(4))))
        for name, fn in runs:
            t = wall(fn, 1) - t_prime
            steps[name] = len(getattr(eng, "spec_records", [])) if name != "greedy" else n - 1
            if r >= 1:
                res.setdefault(name, []).append((n - 1) / t * 1e3)
    say(f"# tokens/s over {n - 1} decoded tokens behind a {S}-token prompt (prefill time subtracted), generate() end to end (drafts= uploads k tokens per step); "
        "oracle = upper bound, adversarial = lower bound; prompt lookup on random weights is shown for completeness only")
    gt = statistics.median(res["greedy"])
    for name, v in res.items():
        say(f"  {name:<20s} {statistics.median(v):8.0f} tok/s   x{statistics.median(v) / gt:.2f}   ({steps[name]} steps)")
    k4 = statistics.median(res["oracle k=4"])
    say(f"acceptance on speed (oracle drafts, k = 4, > greedy in the same run): {k4:.0f} vs {gt:.0f} tok/s: "
        f"{'HOLDS, margin x%.2f' % (k4 / gt) if k4 > gt else 'DOES NOT HOLD'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
