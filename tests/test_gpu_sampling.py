"""Sampled decoding on the GPU (ABI 10): the sampler kernel against the host restatement of the contract (tests/_sampling_ref.py),
its edge cases and its distribution, agreement with the greedy argmax kernels, the sampled steps against the standalone kernel on
their own logits, and the Python entry points."""
import numpy as np
import pytest
import torch

from _sampling_ref import greedy, sample_row, warped_probs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GRID = [(t, k, p) for t in (0.6, 1.0, 1.5) for k in (0, 1, 5, 50) for p in (0.05, 0.5, 0.9, 1.0)]


def _rows(params):
    from onebit_amd.sampling import SampleParamsStruct
    arr = (SampleParamsStruct * len(params))(*[SampleParamsStruct(*p) for p in params])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).reshape(len(params), 32).to(DEV)


def _run(logits16: np.ndarray, params, positions):
    from onebit_amd.sampling import sample_logits
    lg = torch.from_numpy(np.ascontiguousarray(logits16)).to(DEV)
    out = sample_logits(lg, _rows(params), torch.tensor(positions, dtype=torch.int32))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("V", [1, 7, 50, 32000, 32001, 65536])
def test_kernel_matches_host_reference(V):
    rng = np.random.default_rng(V)
    grid = GRID + [(1.0, V + 3, 1.0), (0.8, V + 1, 0.9)]
    params, pos = [], []
    for (t, k, p) in grid:
        for _ in range(2):
            seed = int(rng.integers(0, 2 ** 63))
            params.append((1, t, k, p, seed & 0xFFFFFFFF, seed >> 32, int(rng.integers(0, 2 ** 32)), 0))
            pos.append(int(rng.integers(0, 2 ** 31 - 2)))
    R = len(params)
    logits = (rng.standard_normal((R, V)) * rng.uniform(0.5, 4.0, (R, 1))).astype(np.float16)
    got = _run(logits, params, pos)
    amb = 0
    for r in range(R):
        _, t, k, p, lo, hi, stream, _ = params[r]
        tok, keep, ambiguous = sample_row(logits[r], 1, t, k, p, lo | (hi << 32), stream, pos[r])
        assert 0 <= got[r] < V
        if ambiguous:
            amb += 1
            continue
        if keep is not None:
            assert keep[got[r]], (r, params[r])                          # never outside the kept set
        assert got[r] == tok, (r, params[r], pos[r], got[r], tok)
    assert amb <= max(1, R // 100), amb


def test_adversarial_rows():
    V = 64
    ninf, nan, inf = np.float16(-np.inf), np.float16(np.nan), np.float16(np.inf)
    rows = [np.zeros(V, np.float16),                                               # all ties
            np.where(np.arange(V) % 3 == 0, ninf, np.float16(1.5)).astype(np.float16),
            np.where(np.arange(V) % 2 == 0, nan, np.float16(-2.0)).astype(np.float16),
            np.full(V, nan, np.float16), np.full(V, ninf, np.float16),
            np.where(np.arange(V) == 41, inf, np.float16(3.0)).astype(np.float16),
            np.where(np.arange(V) % 2 == 0, np.float16(65504), np.float16(-65504)).astype(np.float16),
            np.full(V, np.float16(-1.0), np.float16)]
    rows[2][5] = nan
    rows[7][9], rows[7][20] = np.float16(-0.0), np.float16(0.0)            # max 0: -0 first, then +0 -- equal, as argmax has it
    params, logits, pos = [], [], []
    for i, x in enumerate(rows):
        for (ds, t, k, p) in [(0, 1.0, 0, 1.0), (1, 1.0, 0, 1.0), (1, 0.01, 3, 0.5), (1, 2.0, 1, 0.0), (1, -1.0, 5, 0.9),
                              (1, float("nan"), 0, 1.0), (1, 1.0, -4, float("nan")), (1, 1.0, 10 ** 9, 2.0)]:
            params.append((ds, t, k, p, 17 + i, 3, i, 0))
            logits.append(x)
            pos.append(i * 5)
    logits = np.stack(logits)
    got = _run(logits, params, pos)
    for r in range(len(params)):
        ds, t, k, p, lo, hi, stream, _ = params[r]
        assert 0 <= got[r] < V
        tok, keep, ambiguous = sample_row(logits[r], ds, t, k, p, lo | (hi << 32), stream, pos[r])
        if not ambiguous:
            assert got[r] == tok, (r, params[r], got[r], tok)
    assert got[0] == 0                                   # greedy all-ties: first index
    assert got[5 * 8] == 41 and got[5 * 8 + 1] == 41     # a +inf entry wins
    assert all(got[3 * 8 + j] == 0 and got[4 * 8 + j] == 0 for j in range(8))   # all NaN / all -inf: 0
    assert got[7 * 8] == 9                               # greedy: -0 == +0, first index


def test_distribution_chi_square():
    from scipy import stats
    V, N = 32000, 65536
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(V) * 2.0).astype(np.float16)
    seed = 0x1234567890ABCDEF
    for (t, k, p) in [(0.8, 50, 0.9), (1.0, 0, 1.0), (1.5, 0, 0.5)]:
        params = [(1, t, k, p, seed & 0xFFFFFFFF, seed >> 32, 0, 0)] * N
        from onebit_amd.sampling import sample_logits
        lg = torch.from_numpy(x).to(DEV)[None].expand(N, V)
        got = sample_logits(lg, _rows(params[:1]).expand(N, 32).contiguous(), torch.arange(N, dtype=torch.int32)).cpu().numpy()
        probs, keep = warped_probs(x, t, k, p)
        assert keep[got].all()
        cnt = np.bincount(got, minlength=V).astype(np.float64)
        exp = probs * N
        big = exp >= 5
        obs_b, exp_b = np.append(cnt[big], cnt[~big].sum()), np.append(exp[big], exp[~big].sum())
        if exp_b[-1] < 5:
            obs_b, exp_b = obs_b[:-1], exp_b[:-1]
            exp_b *= obs_b.sum() / exp_b.sum()
        chi2 = ((obs_b - exp_b) ** 2 / exp_b).sum()
        pval = stats.chi2.sf(chi2, len(obs_b) - 1)
        assert pval > 1e-4, (t, k, p, chi2, len(obs_b), pval)


def test_agrees_with_argmax():
    """do_sample = 0 rows, and top_k = 1 rows without a tie at the max, give the greedy token."""
    rng = np.random.default_rng(3)
    V, R = 32000, 24
    logits = (rng.standard_normal((R, V)) * 3).astype(np.float16)
    logits[3, 100] = logits[3, 7] = logits[3].max() + np.float16(1)            # a tie at the max: greedy takes the first index
    params = [(0, 1.0, 0, 1.0, r, 0, r, 0) if r % 2 == 0 else (1, 0.7, 1, 1.0, r, 0, r, 0) for r in range(R)]
    got = _run(logits, params, list(range(R)))
    for r in range(R):
        if r % 2 == 0 or (logits[r] == logits[r].max()).sum() == 1:
            assert got[r] == greedy(logits[r]) == int(np.argmax(logits[r].astype(np.float32))), r
    assert got[2] == greedy(logits[2])


def _tiny_model(vocab=1000, seed=3):
    from onebit_amd.llama import OneBitLlamaConfig, build_synthetic_model
    cfg = OneBitLlamaConfig(vocab_size=vocab, hidden_size=128, intermediate_size=352, num_hidden_layers=2,
                            num_attention_heads=2, max_position_embeddings=256)
    return build_synthetic_model(cfg, seed=seed, device=DEV)


def _mixed_params(n, seed0=11):
    from onebit_amd.sampling import SamplingParams
    grid = [(0.7, 50, 0.9), (1.0, 0, 1.0), (1.3, 5, 1.0), (0.9, 0, 0.5)]
    return [None if i % 3 == 0 else SamplingParams(*grid[i % 4], seed=seed0 + i, stream=i) for i in range(n)]


def test_decode_step_sampled_matches_standalone_kernel():
    """onebit_decode_step_sampled: the token of every step equals onebit_sample_rows on the step's own logits at n = pos + 1,
    and the step writes out_tokens[p] and pos = p + 1 as the greedy step does."""
    import ctypes
    from onebit_amd import _lib
    from onebit_amd.engine import DecodeEngine
    from onebit_amd.sampling import SamplingParams, pack, sample_logits
    model = _tiny_model()
    eng = DecodeEngine(model, max_len=64, use_graph=False, long_context_from=0)
    ids = torch.randint(0, 1000, (1, 7), generator=torch.Generator().manual_seed(1)).to(DEV)
    eng.prime(ids)
    lib = _lib.load()
    for i, sp in enumerate([SamplingParams(0.8, 50, 0.9, seed=5), None, SamplingParams(1.2, 0, 1.0, seed=9, stream=3)] * 4):
        pr = pack([sp], DEV)
        p = int(eng.pos.item())
        st = eng._variants["64" if p < 64 else "short"]
        rc = lib.onebit_decode_step_sampled(ctypes.byref(eng._model), ctypes.byref(st), pr.data_ptr(),
                                            torch.cuda.current_stream(DEV).cuda_stream)
        _lib.check(rc, "onebit_decode_step_sampled")
        torch.cuda.synchronize()
        want = int(sample_logits(eng.buf["logits"][None], pr, [p + 1]).item())
        assert int(eng.token.item()) == want == int(eng.out_tokens[p].item()), (i, p)
        assert int(eng.pos.item()) == p + 1
        if sp is None:
            assert want == int(eng.buf["logits"].float().argmax().item())


def test_batched_step_sampled_matches_standalone_kernel():
    from onebit_amd.engine import BatchedDecodeStep, fp16_view
    from onebit_amd.sampling import pack, sample_logits
    model = _tiny_model()
    B, L = 32, 64
    cache = fp16_view(model).new_cache(B, L)
    step = BatchedDecodeStep(model, cache.layers, B, L, keep_logits=True)
    g = torch.Generator().manual_seed(4)
    step.tokens.copy_(torch.randint(0, 1000, (B,), generator=g).int())
    step.pos.copy_(torch.randint(0, L - 1, (B,), generator=g).int())
    pr = pack(_mixed_params(B), DEV)
    pos0 = step.pos.clone()
    step.launch(params=pr)
    torch.cuda.synchronize()
    got = step.next_tokens.clone()
    want = sample_logits(step.logits, pr, pos0 + 1)
    assert torch.equal(got, want)
    greedy_rows = [b for b in range(B) if b % 3 == 0]
    assert torch.equal(got[greedy_rows].long(), step.logits[greedy_rows].float().argmax(-1))
    step.launch()                                        # the greedy form of the same step (ob_b_argmax_kernel) on the same state
    torch.cuda.synchronize()
    assert torch.equal(step.next_tokens[greedy_rows], got[greedy_rows])


def test_mixed_step_sampled_over_64_rows_matches_standalone_kernel():
    from onebit_amd.engine import MixedStep, fp16_view
    from onebit_amd.sampling import pack, sample_logits
    model = _tiny_model()
    n, L = 70, 64
    cache = fp16_view(model).new_cache(n, L)
    ms = MixedStep(model, cache.layers, n, L, max_rows=256, keep_logits=True)
    g = torch.Generator().manual_seed(6)
    items = []
    for i in range(n):
        k = 1 + i % 4
        items.append((i, 0, torch.randint(0, 1000, (k,), generator=g).tolist()))
    pr = pack(_mixed_params(n), DEV)
    got = ms.launch(items, params=pr).clone()
    torch.cuda.synchronize()
    want = sample_logits(ms.logits[:n], pr, [len(it[2]) for it in items])
    assert torch.equal(got, want)
    greedy_rows = [i for i in range(n) if i % 3 == 0]
    assert torch.equal(got[greedy_rows].long(), ms.logits[greedy_rows].float().argmax(-1))
    greedy = ms.launch(items).clone()                    # the greedy form of the same step rewrites the same cache rows
    torch.cuda.synchronize()
    assert torch.equal(greedy[greedy_rows], got[greedy_rows])


def test_module_generate_do_sample():
    model = _tiny_model()
    ids = torch.randint(0, 1000, (3, 5), generator=torch.Generator().manual_seed(2)).to(DEV)
    greedy_out = model.generate(ids, 6)
    a = model.generate(ids, 6, do_sample=True, temperature=1.5, top_k=0, seed=123)
    b = model.generate(ids, 6, do_sample=True, temperature=1.5, top_k=0, seed=123)
    c = model.generate(ids, 6, do_sample=True, temperature=1.5, top_k=0, seed=124)
    assert torch.equal(a, b) and not torch.equal(a, c) and a.shape == greedy_out.shape
    assert torch.equal(a[:, :5], ids) and int(a.max()) < 1000
    assert torch.equal(model.generate(ids, 6, do_sample=True, top_k=1, seed=7), greedy_out)     # top_k = 1 is greedy (no ties here)
    e = model.generate(ids, 6, do_sample=True, temperature=1.5, top_k=0, seed=123, eos_token_id=int(a[0, 6]), pad_token_id=0)
    assert e[0, 6] == a[0, 6] and (e[0, 7:] == 0).all()


def test_decode_engine_sampled_graphs_match_standalone_kernel():
    """DecodeEngine.prime / step with sampling: the first token from the sampled mixed step, later ones from the sampled graphs
    (short, position < 64, key-block forms, captured on first use); every token equals onebit_sample_rows on that step's logits
    at n = position, and generate() gives the same tokens."""
    from onebit_amd.engine import DecodeEngine
    from onebit_amd.sampling import SamplingParams, pack, sample_logits
    model = _tiny_model()
    eng = DecodeEngine(model, max_len=256, long_context_from=160)
    sp = SamplingParams(0.9, 50, 0.9, seed=77, stream=2)
    pr = pack([sp], DEV)
    ids = torch.randint(0, 1000, (1, 30), generator=torch.Generator().manual_seed(9)).to(DEV)
    first = eng.prime(ids, sampling=sp)
    assert first == int(sample_logits(eng._mixed.logits[:1], pr, [30]).item())
    toks = [first]
    for p in range(30, 200):
        eng.step()
        torch.cuda.synchronize()
        t = int(eng.token.item())
        assert t == int(sample_logits(eng.buf["logits"][None], pr, [p + 1]).item()), p
        toks.append(t)
    sampled = {k for k, s in eng._graphs if s}
    assert {"64", "short"} <= sampled and any(isinstance(k, tuple) for k in sampled)
    assert eng.generate(ids, len(toks), sampling=sp)[0, 30:].tolist() == toks
    g = eng.generate(ids, 40)[0, 30:].tolist()                       # greedy again afterwards: the greedy graphs
    assert g == eng.generate(ids, 40)[0, 30:].tolist() and eng._sampled is False


def _batcher_run(model, reqs, order=None, **kw):
    from onebit_amd.serving import ContinuousBatcher
    cb = ContinuousBatcher(model, max_batch=kw.pop("max_batch", 8), max_len=128, **kw)
    order = order if order is not None else list(range(len(reqs)))
    rid = {}
    for i in order:
        prompt, n, sp = reqs[i]
        rid[i] = cb.add_request(prompt, n, sampling=sp)
    out = cb.run()
    return [out[rid[i]] for i in range(len(reqs))], cb


def test_continuous_batcher_sampling():
    from onebit_amd.sampling import SamplingParams
    model = _tiny_model()
    g = torch.Generator().manual_seed(12)
    prompts = [torch.randint(0, 1000, (n,), generator=g).tolist() for n in (5, 9, 3, 12, 7, 4)]
    sps = [None, SamplingParams(0.8, 50, 0.9, seed=1), None, SamplingParams(1.3, 0, 1.0, seed=2, stream=5),
           SamplingParams(1.0, 5, 0.5, seed=3), None]
    reqs = [(p, 20, sp) for p, sp in zip(prompts, sps)]
    mixed, cb = _batcher_run(model, reqs)
    assert cb.graph_steps > 0 and cb._graph_s is not None and cb._graph is None      # every decode-only step carried a sampled request
    greedy, _ = _batcher_run(model, [(p, n, None) for p, n, _ in reqs])
    for i, sp in enumerate(sps):
        if sp is None:
            assert mixed[i] == greedy[i], i                          # greedy requests next to sampled ones: unchanged
    assert any(mixed[i] != greedy[i] for i in range(6) if sps[i] is not None)
    rev, _ = _batcher_run(model, reqs, order=list(reversed(range(6))))
    assert rev == mixed                                              # the other submission order (all admitted in the first step)
    burst, cbb = _batcher_run(model, reqs, max_burst=4)
    assert burst == mixed and cbb._graph_fb_s is not None            # decode bursts: the same tokens
    torch_path, _ = _batcher_run(model, reqs, native=False, use_graph=False)
    for i, sp in enumerate(sps):                                     # the torch-glue path samples through sample_logits
        assert len(torch_path[i]) == 20 and max(torch_path[i]) < 1000


def _perturbed(model, prefix, n, sp, stream):
    """The module path's fp32 scores + Gumbel noise at the next token (for the near-tie escape)."""
    from _sampling_ref import gumbel, scores
    lg = model(torch.tensor([prefix], device=DEV))[0, -1].half().cpu().numpy()
    s = scores(lg, sp.temperature).astype(np.float64)
    return s + gumbel(len(s), sp.seed & 0xFFFFFFFF, sp.seed >> 32, stream, n)


@pytest.mark.parametrize("B", [1, 3])
def test_generate_native_do_sample(B):
    from onebit_amd.llama import OneBitLlamaConfig, build_synthetic_model
    from onebit_amd.sampling import SamplingParams
    cfg = OneBitLlamaConfig(vocab_size=64, hidden_size=512, intermediate_size=1408, num_hidden_layers=2, num_attention_heads=4,
                            max_position_embeddings=256)
    model = build_synthetic_model(cfg, seed=23, device=DEV)
    ids = torch.randint(0, cfg.vocab_size, (B, 9), generator=torch.Generator().manual_seed(B)).to(DEV)
    kw = dict(do_sample=True, temperature=1.2, top_k=0, top_p=1.0)
    a = model.generate_native(ids, 24, seed=31, **kw)
    assert torch.equal(a, model.generate_native(ids, 24, seed=31, **kw))             # repeatable
    assert not torch.equal(a, model.generate_native(ids, 24, seed=32, **kw))         # another seed, other tokens
    ref = model.generate(ids, 24, seed=31, **kw)
    assert a.shape == ref.shape and torch.equal(a[:, :9], ids)
    sp = SamplingParams(1.2, 0, 1.0, seed=31)
    same = True
    for r in range(B):
        ra, rb = a[r].tolist(), ref[r].tolist()
        if ra != rb:
            j = next(i for i in range(len(ra)) if ra[i] != rb[i])
            sc = _perturbed(model, rb[:j], j, sp, r)              # token j of the sequence is drawn at n = j
            assert abs(sc[ra[j]] - sc[rb[j]]) < 2e-2 * max(1.0, float(np.abs(sc[np.isfinite(sc)]).max())), (r, j)
            same = False
    if same:
        eos = int(ref[0, 9 + 5])
        ref_e = model.generate(ids, 24, seed=31, eos_token_id=eos, pad_token_id=0, **kw)
        got_e = model.generate_native(ids, 24, seed=31, eos_token_id=eos, pad_token_id=0, **kw)
        assert torch.equal(got_e, ref_e)
        assert B > 1 or int(ref_e[0, -1]) == eos
