"""``onebit_mixed_step`` against the REFERENCE's recorded logits (not against this repository's module path, which
tests/test_gpu_mixed.py compares it with at 1e-2 x logit scale): every comparison goes through ``_parity_log.check`` with the bar
derived from the fixture's own goldens, ``max(1.6 x the reference's fp16-vs-fp32 gap + half an fp16 ulp, 2e-3 x scale)`` -- the bar of
the module path, ``DecodeEngine``, ``BatchedDecodeStep``, the K-sharded decoder and the speculative verify pass.  Default routes
only: no environment switch is set here.

  * 7B widths (``model_wide_c.npz``): the 4096-token prompt whose logits the reference recorded at 16 positions, cut after each
    recorded position -- chunks of 93, 1076, 748, 190, 470, 166, 548, 12 and 786 rows, each on a non-empty past, then 7 decode rows at
    a context of ~4090 keys (16 splits of 256) -- with twelve of the 32 batch sequences riding along as 6-row segments and decode rows:
    one step in every route of ``onebit_mixed.hip`` (tests/_mixed_plan.py ``classify``); then the same prompt in another slot as chunks
    of 2107 + 1982 + 7 rows with lm_head on up to 2015 rows of a chunk.  Caches poisoned with NaN, again before every step from each item's start on: a key read
    beyond past + n shows.
  * the fixtures' short prompts (tiny b, tiny with attention bias and 3 layers, 13B widths, 7B widths): whole, as 3 + rest, both
    at once out of phase, every row's logits (``k``) and the teacher-forced decode steps; at 13B widths the 8 batch sequences as
    one 48-row step and two decode-only steps.
  * 32 layers at 7B widths (``model_wide_d.npz``).

tests/test_mixed_plan_cpu.py checks the schedules and that the driver (``_mixed_plan.drive``) fails on planted faults.  Measured
error / gap per compared group: profiles/mixed_reference_parity.txt."""
import os

import numpy as np
import pytest
import torch

import _mixed_plan as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _mixed(model, n_slots, max_len, max_rows):
    """A MixedStep on caches full of NaN, the ``launch`` the driver calls and its ``before_step`` hook."""
    from onebit_amd.engine import MixedStep
    cfg, dev = model.config, torch.device(DEV)
    shape = (n_slots, cfg.num_key_value_heads, max_len, cfg.head_dim)
    caches = [(torch.full(shape, float("nan"), dtype=torch.float16, device=dev), torch.full(shape, float("nan"), dtype=torch.float16, device=dev))
              for _ in range(cfg.num_hidden_layers)]
    ms = MixedStep(model, caches, n_slots=n_slots, max_len=max_len, max_rows=max_rows, keep_logits=True)

    def poison(si, st):
        # before every step: NaN from each item's ``start`` to the end of its slot -- what the step does not write itself (a reused
        # slot's previous sequence included) reads as NaN, so a key read beyond past + n shows in every step, not only on first use
        for slot, start, toks, k in st.items:
            for kc, vc in caches:
                kc[slot, :, start:] = float("nan")
                vc[slot, :, start:] = float("nan")

    def launch(items):
        n_out = sum(it[3] for it in items)
        nxt = ms.launch(items)
        torch.cuda.synchronize()
        assert nxt.shape[0] == n_out
        return ms.logits[:n_out].float().cpu().numpy(), nxt.cpu().numpy()
    return caches, launch, poison


def _synthetic(golden_dir, name, widths):
    from onebit_amd.llama import OneBitLlamaConfig, OneBitLlamaForCausalLM, synthetic_state_dict
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = OneBitLlamaConfig(**{k[4:]: int(z[k]) for k in z.files if k.startswith("cfg_")})
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.head_dim, cfg.num_hidden_layers) == widths
    model = OneBitLlamaForCausalLM(cfg, torch.float16)
    model.load_state_dict(synthetic_state_dict(cfg, seed=int(z["seed"]), dtype=torch.float16, device="cpu"))
    return z, model.to(torch.device(DEV)).eval()


def _tiny(golden_dir, name):
    from onebit_amd.llama import OneBitLlamaConfig, OneBitLlamaForCausalLM
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    model = OneBitLlamaForCausalLM(OneBitLlamaConfig(**{k[4:]: int(z[k]) for k in z.files if k.startswith("cfg_")}), torch.float16)
    model.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")})
    return z, model.to(torch.device(DEV)).eval()


@pytest.fixture(scope="module")
def wide(golden_dir):
    return _synthetic(golden_dir, "model_wide_c", (4096, 11008, 128, 2))


@pytest.fixture(scope="module")
def wide_long(wide):
    """ONE MixedStep for both variants of the long prompt: 6 slots of 4096 positions (128 MB of cache per slot), room for variant B's
    2107-row step from the start (variant A alone needs 1083 rows)."""
    z, model = wide
    return _mixed(model, n_slots=6, max_len=4096, max_rows=2107)


def _long_positions(rec):
    return sorted(i[0] for r in rec if r["array"] == "long_logits" for i in r["index"])


def test_long_prompt_cut_at_the_recorded_positions_with_riders(wide, wide_long):
    """Schedule A in slot 0, batch sequences riding in slots 1 .. 3: 18 steps of 99, 1083, 756, 193, 478, 174, 556, 15, 794 rows,
    then 9 / 9 / 4 / ... rows with the long prompt's decode row at positions 4089 .. 4095."""
    z, model = wide
    caches, launch, poison = wide_long
    steps = P.with_riders(P.long_schedule(z, "A", slot=0), z, [1, 2, 3])
    rec = P.drive(launch, steps, z, "model_wide_c", "MixedStep long A + riders", before_step=poison)
    assert _long_positions(rec) == list(range(16))
    assert {r["regime"] for r in rec if r["array"] == "long_logits"} == set(P.REGIMES)
    riders = {i for r in rec if r["array"] == "batch_logits" for i in r["index"]}
    assert riders == {(b, ph) for b in range(12) for ph in range(4)}
    for kc, vc in caches:                                                      # slot 5 was named by no item: nothing wrote there
        assert bool(torch.isnan(kc[5]).all()) and bool(torch.isnan(vc[5]).all())


def test_long_prompt_in_three_chunks_tail_through_the_flash_kernel(wide, wide_long):
    """Schedule B in slot 4 of the same MixedStep : 2107 + 1982 + 7 rows, all 16 recorded positions,
    the last 7 as rows of ONE chunk (k = 7); 3535 output rows in all, each one's token = the argmax of its logits."""
    z, model = wide
    caches, launch, poison = wide_long
    rec = P.drive(launch, P.long_schedule(z, "B", slot=4), z, "model_wide_c", "MixedStep long B", before_step=poison)
    assert _long_positions(rec) == list(range(16))
    assert [r["T"] for r in rec] == [2107, 1982, 7]


def _short_runs(z, n_slots):
    S = z["input_ids"].shape[1]
    assert n_slots >= 4
    return [("whole", P.short_schedule(z, 0)),
            ("3+rest", P.short_schedule(z, 1, [3, S - 3])),
            ("both, two steps apart", P.merge(P.short_schedule(z, 2, [3, S - 3]), P.short_schedule(z, 3), offset=2))]


# (model_tiny_a is not among them: its intermediate_size 688 makes down_proj's K no multiple of 32, which the native engines refuse when
#  they bind the model -- test_tiny_a_is_refused_when_the_step_binds_the_model below; its recorded logits pin the module path only)
@pytest.mark.parametrize("name", ["model_tiny_b", "model_tiny_bias", "model_wide_e", "model_wide_c"])
def test_short_prompts_every_row_and_decode_steps(golden_dir, request, name):
    if name == "model_wide_c":
        z, model = request.getfixturevalue("wide")
    elif name == "model_wide_e":
        z, model = _synthetic(golden_dir, name, (5120, 13824, 128, 2))
    else:
        z, model = _tiny(golden_dir, name)
        assert (model.model.layers[0].self_attn.q_proj.bias is not None) == (name == "model_tiny_bias")
        assert model.config.num_hidden_layers == (3 if name == "model_tiny_bias" else 2)
    S, nd = z["input_ids"].shape[1], z["decode_logits_f16"].shape[1]
    n_slots = 8 if name == "model_wide_e" else 4
    _, launch, poison = _mixed(model, n_slots=n_slots, max_len=32, max_rows=64)
    for what, steps in _short_runs(z, n_slots):
        rec = P.drive(launch, steps, z, name, "MixedStep short prompt " + what, before_step=poison)
        n = 2 if what.startswith("both") else 1
        assert sorted(i for r in rec if r["array"] == "prefill_logits" for i in r["index"]) == sorted([(0, p) for p in range(S)] * n)
        assert sorted(i for r in rec if r["array"] == "decode_logits" for i in r["index"]) == sorted([(0, i) for i in range(nd)] * n)
    if name == "model_wide_e":
        # the eight batch sequences entering together (48 rows, last rows = batch_logits[:, 0]), then two decode-only steps (no segment)
        steps = P.batch_schedule(z, list(range(8)))
        assert [P.rows_of(st) for st in steps] == [48, 8, 8] and all(len(it[2]) == 1 for st in steps[1:] for it in st.items)
        rec = P.drive(launch, steps, z, name, "MixedStep 8 sequences", before_step=poison)
        assert sorted(i for r in rec for i in r["index"]) == [(b, i) for b in range(8) for i in range(3)]


def test_32_layers(golden_dir):
    """``model_wide_d``: 7B widths, all 32 decoder layers -- the 12-token prompt with k = 12, then the two recorded decode steps."""
    z, model = _synthetic(golden_dir, "model_wide_d", (4096, 11008, 128, 32))
    _, launch, poison = _mixed(model, n_slots=2, max_len=32, max_rows=64)
    steps = P.short_schedule(z, 1)
    assert [(P.rows_of(st), st.items[0][3]) for st in steps] == [(12, 12), (1, 1), (1, 1)]
    rec = P.drive(launch, steps, z, "model_wide_d", "MixedStep 32 layers", before_step=poison)
    assert len(rec) == 3


def test_tiny_a_is_refused_when_the_step_binds_the_model(golden_dir):
    """``model_tiny_a`` has intermediate_size 688: down_proj's K is no multiple of 32, and the native step refuses the model when it binds it,
    before any launch -- there are no mixed-step logits to hold to this fixture (the serving layer falls back to the module path for
    it, tests/test_gpu_serving.py)."""
    from onebit_amd.engine import MixedStep
    z, model = _tiny(golden_dir, "model_tiny_a")
    cfg, dev = model.config, torch.device(DEV)
    assert cfg.intermediate_size == 688
    shape = (2, cfg.num_key_value_heads, 32, cfg.head_dim)
    caches = [(torch.zeros(shape, dtype=torch.float16, device=dev), torch.zeros(shape, dtype=torch.float16, device=dev)) for _ in range(cfg.num_hidden_layers)]
    with pytest.raises(ValueError, match="in_features=688 is not a multiple of 32"):
        MixedStep(model, caches, n_slots=2, max_len=32, max_rows=64, keep_logits=True)
