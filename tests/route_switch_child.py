"""Child process of tests/test_gpu_route_switches.py: runs the named workloads once, in a fresh interpreter whose environment
carries the switch under test (the library reads every OB_* switch once per process).

    python tests/route_switch_child.py OUT_DIR linear,gemv,...

Each workload asserts its own bars (the oracle, or the reference's logits for the model-level ones), writes its outputs as .npy
files and the kernels it launched -- name, grid and block of every dispatch the profiler saw -- as kernels.json under
OUT_DIR/<workload>/, and prints one ``ok <workload>`` line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(ROOT, "tests", "golden")

# (T, K, N, bias): the route boundaries of test_forward_shape_sweep_hits_every_kernel_route (decode GEMV, skinny 16 / 32 / 64-token
# tiles, 64-row GEMM tiles, 128 x 128 prefill tiles, K % 128 != 0), the forced-route child's ragged 256 x 256 shapes, and K-sliced
# shapes small enough for the oracle: 1 tile x 4 slices, 6 tiles x 2 slices, 48 rows (below the K-slice row floor)
LINEAR_SHAPES = [(T, K, N, False) for T in (1, 2, 16, 17, 32, 33, 64, 65, 129) for (K, N) in ((512, 64), (640, 200))]
LINEAR_SHAPES += [(17, 96, 48, False), (65, 96, 48, False), (1, 2560, 72, False), (1, 4096, 11008, False),
                  (300, 512, 260, False), (192, 256, 40, False),
                  (66, 4096, 256, True), (130, 2048, 520, False), (48, 2048, 264, False)]


def wl_linear():
    """onebit_linear_forward through BitLinearInf against the oracle (fp16; y and the pre-LayerNorm u)"""
    from oracle.oracle import COracle
    from test_gpu_parity import _check_f16, _check_f16_sliced, _make_layer, _t
    co = COracle()
    rng = np.random.default_rng(2024)
    out = {}
    for i, (T, K, N, bias) in enumerate(LINEAR_SHAPES):
        packed = rng.integers(0, 256, (N, K // 8), dtype=np.uint8).view(np.int8)
        h = (0.1 * (0.5 + rng.random(K)) * np.where(rng.random(K) < 0.1, -1, 1)).astype(np.float16)
        g = (0.1 * (0.5 + rng.random(N)) * np.where(rng.random(N) < 0.1, -1, 1)).astype(np.float16)
        b = (0.1 * rng.standard_normal(N)).astype(np.float16) if bias else None
        x = rng.standard_normal((T, K)).astype(np.float16)
        y_ref, u_ref = co.forward_f16(packed, x, h, g, b, return_pre_ln=True)
        m = _make_layer(K, N, torch.float16, DEV, packed, h, g, b)
        y = m(_t(x, DEV)).cpu().numpy()
        m.layernorm = torch.nn.Identity()
        m.bias = None
        u = m(_t(x, DEV)).cpu().numpy()
        # sums over K >= 2048 may cancel far below their own scale: the K-sliced test's element bar
        (_check_f16_sliced if K >= 2048 and T > 1 else _check_f16)(y, u, y_ref, u_ref, (T, K, N))
        out[f"y{i}"], out[f"u{i}"] = y, u
    return out


def wl_gemv():
    """the fused decode GEMV chain at 7B widths (o_proj alone, gate | up, down) against the oracle: the test itself, with every
    output the chain writes recorded"""
    import onebit_amd.engine as engine
    from oracle.oracle import COracle
    import test_gpu_fullsize
    rec = []
    plain = engine.fused_gemv

    def recording(mods, outs, prologue, *a, **kw):
        r = plain(mods, outs, prologue, *a, **kw)
        rec.extend(o.detach().cpu().numpy().copy() for o in outs)
        return r
    engine.fused_gemv = recording
    try:
        test_gpu_fullsize.test_fused_gemv_chain_vs_oracle(COracle(), 4096, 11008)
    finally:
        engine.fused_gemv = plain
    assert rec
    return {f"out{i}": a for i, a in enumerate(rec)}


def _wide(name):
    """the reference goldens' model: weights regenerated from the fixture's seed (tests/golden/gen_goldens_model_wide.py)"""
    from onebit_amd.llama import OneBitLlamaConfig, OneBitLlamaForCausalLM, synthetic_state_dict
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = OneBitLlamaConfig(**{k[4:]: int(z[k]) for k in z.files if k.startswith("cfg_")})
    model = OneBitLlamaForCausalLM(cfg, torch.float16)
    model.load_state_dict(synthetic_state_dict(cfg, seed=int(z["seed"]), dtype=torch.float16, device="cpu"))
    return z, model.to(DEV).eval()


def wl_decode():
    """DecodeEngine on model_wide_c against the reference's logits: as is (positions 12..15: the blind-64 attention), on the
    key-block attention, and one step at position 92 of the reference's long prompt (the 128-row blind window)"""
    from _parity_log import check, loose_tol
    from onebit_amd.engine import DecodeEngine
    z, model = _wide("model_wide_c")
    ids = torch.from_numpy(z["input_ids"]).to(DEV)
    toks = z["greedy_f16"][0]
    r16, r32 = z["decode_logits_f16"], z["decode_logits_f32"]
    bar = max(loose_tol(r16, r32), loose_tol(z["prefill_logits_f16"], z["prefill_logits_f32"]))
    out = {}
    for name, kw in (("plain", dict(max_len=32)), ("keyblock", dict(max_len=64, long_context_from=4, long_attention="keyblock", attn_chunk=64))):
        eng = DecodeEngine(model, use_graph=False, **kw)
        eng.prefill(ids)
        assert eng.first_token == int(toks[0])
        for i in range(4):
            eng.set_state(int(toks[i]), ids.shape[1] + i)
            eng.step()
            lg = eng.logits().cpu().numpy()
            check("model_wide_c", "decode_logits", f"route switch: DecodeEngine {name} step {i}", lg, r16[0, i], r32[0, i], loose=bar)
            out[f"{name}{i}"] = lg
    p = int(z["long_pos"][0])
    assert 64 < p < 128
    lids = z["long_ids"][0]
    eng = DecodeEngine(model, max_len=128, use_graph=False)
    eng.prefill(torch.from_numpy(lids[None, :p]).to(DEV))
    eng.set_state(int(lids[p]), p)
    eng.step()
    lg = eng.logits().cpu().numpy()
    l16, l32 = z["long_logits_f16"], z["long_logits_f32"]
    check("model_wide_c", "long_logits", f"route switch: DecodeEngine position {p}", lg, l16[0], l32[0], loose=loose_tol(l16, l32))
    out["long"] = lg
    return out


def wl_batched():
    """BatchedDecodeStep against the reference's batched logits: model_wide_c (7B widths, 32 slots) and model_wide_e (13B widths,
    8 slots), each with the one-workgroup attention and the key-block attention"""
    from _parity_log import check, loose_tol
    from onebit_amd.engine import BatchedDecodeStep
    out = {}
    for name in ("model_wide_c", "model_wide_e"):
        z, model = _wide(name)
        bids = torch.from_numpy(z["batch_ids"]).to(DEV)
        B, S = bids.shape
        ref16, ref32 = z["batch_logits_f16"], z["batch_logits_f32"]
        bar = loose_tol(ref16, ref32)
        toks = z["batch_greedy_f16"]
        for splits in (0, 1):
            cache = model.new_cache(B, 16)
            lg = model(bids, cache)[:, -1].cpu().numpy()
            check(name, "batch_prefill", "route switch: module path", lg, ref16[:, 0], ref32[:, 0], loose=bar)
            step = BatchedDecodeStep(model, cache.layers, B, 16, sample=True, keep_logits=True, attn_splits=splits, attn_chunk=64)
            out[f"{name}_s{splits}_prefill"] = lg
            for i in range(ref16.shape[1] - 1):
                step.tokens.copy_(torch.from_numpy(toks[:, i].astype(np.int32)))
                step.pos.fill_(S + i)
                step.launch()
                torch.cuda.synchronize()
                got = step.logits.float().cpu().numpy()
                check(name, "batch_decode", f"route switch: BatchedDecodeStep splits={splits} step {i}", got, ref16[:, 1 + i], ref32[:, 1 + i],
                      loose=bar)
                out[f"{name}_s{splits}_step{i}"] = got
        del model
        torch.cuda.empty_cache()
    return out


# rows of one mixed step at 13B widths: both sides of the single-launch limit (64 / 65), skinny passes (200: q|k|v not grouped),
# the grouped launches just above the pass limit (321), a grouped launch with a 31-row tail (543), and 700 rows
MIXED_ROWS = (64, 65, 200, 321, 543, 700)


def wl_mixed():
    """onebit_mixed_step at 13B widths against the module path (as test_gpu_mixed.py::test_mixed_step_mid_size_routes), and on
    model_wide_c 32 six-token prompts in one step against the reference's logits of their first position"""
    from _parity_log import check, loose_tol
    from onebit_amd.engine import MixedStep
    from onebit_amd.llama import OneBitLlamaConfig, build_synthetic_model
    out = {}
    cfg = OneBitLlamaConfig(vocab_size=512, hidden_size=5120, intermediate_size=13824, num_hidden_layers=2,
                            num_attention_heads=40, max_position_embeddings=1024)
    model = build_synthetic_model(cfg, seed=29, device=DEV)
    slots, max_len, n_dec = 4, 800, 3
    shape = (slots, cfg.num_key_value_heads, max_len, cfg.head_dim)
    for rows in MIXED_ROWS:
        caches = [(torch.zeros(shape, dtype=torch.float16, device=DEV), torch.zeros(shape, dtype=torch.float16, device=DEV))
                  for _ in range(cfg.num_hidden_layers)]
        ms = MixedStep(model, caches, slots, max_len, max_rows=1024, keep_logits=True)
        g = torch.Generator().manual_seed(rows)
        seqs = {s: torch.randint(0, 512, (n,), generator=g).tolist() for s, n in [(0, 20), (1, 7), (2, 33), (3, rows - n_dec)]}
        ms.launch([(s, 0, seqs[s][:-1]) for s in range(n_dec)])
        torch.cuda.synchronize()
        items = [(s, len(seqs[s]) - 1, seqs[s][-1:]) for s in range(n_dec)] + [(3, 0, seqs[3])]
        assert sum(len(t) for _, _, t in items) == rows
        nxt = ms.launch(items).clone()
        torch.cuda.synchronize()
        lg = ms.logits[:len(items)].float()
        for i, (slot, start, toks) in enumerate(items):
            ref = model(torch.tensor([seqs[slot]], device=DEV))[0, -1].float()
            scale = float(ref.abs().max())
            assert float((lg[i] - ref).abs().max()) < 1e-2 * scale, (rows, i, slot)
            assert int(nxt[i]) == int(lg[i].argmax())
        out[f"rows{rows}"] = lg.cpu().numpy()
        del ms, caches
    del model
    torch.cuda.empty_cache()
    z, model = _wide("model_wide_c")
    bids = z["batch_ids"]
    B, S = bids.shape
    c = model.config
    shape = (B, c.num_key_value_heads, 16, c.head_dim)
    caches = [(torch.zeros(shape, dtype=torch.float16, device=DEV), torch.zeros(shape, dtype=torch.float16, device=DEV))
              for _ in range(c.num_hidden_layers)]
    ms = MixedStep(model, caches, B, 16, keep_logits=True)
    ms.launch([(b, 0, bids[b].tolist()) for b in range(B)])               # 192 rows: skinny passes
    torch.cuda.synchronize()
    got = ms.logits[:B].float().cpu().numpy()
    ref16, ref32 = z["batch_logits_f16"], z["batch_logits_f32"]
    check("model_wide_c", "batch_prefill", "route switch: mixed step, 32 prompts", got, ref16[:, 0], ref32[:, 0], loose=loose_tol(ref16, ref32))
    out["wide_c"] = got
    return out


def wl_train():
    """the fp16 train-mode layer (forward and backward) against its fp64 restatement, at the shapes of test_gpu_train.py, and
    element by element over the case table of test_gpu_train_elementwise.py"""
    import test_gpu_train
    import test_gpu_train_elementwise
    from _train_ref import CASE_IDS
    for (T, K, N) in ((256, 1024, 768), (77, 200, 136), (5, 24, 8), (300, 1000, 520), (129, 130, 131)):
        test_gpu_train.test_fp16_against_restatement_in_fp64(T, K, N)
    for case_id in CASE_IDS:
        test_gpu_train_elementwise.test_elementwise_parity(case_id, "float16")
    return {}


WORKLOADS = {"linear": wl_linear, "gemv": wl_gemv, "decode": wl_decode, "batched": wl_batched, "mixed": wl_mixed, "train": wl_train}


def _kernels(trace_path):
    """name, grid and block of every kernel dispatch in a torch.profiler chrome trace"""
    with open(trace_path) as f:
        events = json.load(f).get("traceEvents", [])
    ks = []
    for e in events:
        if str(e.get("cat", "")).lower() != "kernel":
            continue
        a = e.get("args", {})
        ks.append([e.get("name", ""), a.get("grid"), a.get("block")])
    return ks


def main():
    from torch.profiler import ProfilerActivity, profile
    from onebit_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()                          # the native library must be present: no fallback
    out_dir, names = sys.argv[1], sys.argv[2].split(",")
    for name in names:
        d = os.path.join(out_dir, name)
        os.makedirs(d, exist_ok=True)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            arrays = WORKLOADS[name]()
            torch.cuda.synchronize()
        for k, a in arrays.items():
            np.save(os.path.join(d, k + ".npy"), np.ascontiguousarray(a))
        trace = os.path.join(d, "trace.json")
        prof.export_chrome_trace(trace)
        ks = _kernels(trace)
        os.remove(trace)
        with open(os.path.join(d, "kernels.json"), "w") as f:
            json.dump(ks, f)
        print("ok", name, len(ks), flush=True)


if __name__ == "__main__":
    main()
