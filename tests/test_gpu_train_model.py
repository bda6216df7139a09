"""The train-mode model (onebit_amd/train_model.py: OneBitLlamaForCausalLMTrain) on the configs of tests/golden/train_model_tiny.npz.

Truth is tests/_train_model_ref.py evaluated in float64 on the CPU (pinned to the reference's recorded numbers by
tests/test_train_model_cpu.py); the bars are ``_train_ref.MARGIN x`` the distance to it of the same restatement evaluated on the CPU in
the model's dtype, per tensor, for max |a - b| / rms(b) and the relative L2: logits, every hidden state, the loss and the recorded
gradients.  No number comes from the kernels."""
import pytest
import torch

import _train_model_ref as M
import _train_ref as R

from onebit_amd.llama import OneBitLlamaConfig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = [("float32", "eager"), ("float16", "hip"), ("float16", "eager")]


def _model(record, dtype, attention, **kw):
    from onebit_amd.train_model import OneBitLlamaForCausalLMTrain
    return OneBitLlamaForCausalLMTrain(OneBitLlamaConfig(**M.CONFIGS[record]), dtype=dtype, attention=attention, **kw)


def _run(record, dtype, attention, **kw):
    cfg = M.CONFIGS[record]
    ids, labels = M.make_batch(cfg, M.SEEDS[record])
    model = _model(record, dtype, attention, **kw)
    return M.run_model(model, M.make_params(cfg, M.SEEDS[record]), ids, labels, dtype, DEV), model


def _within(what, got, truth, own, names):
    bad = {}
    for n in names:
        assert got[n].shape == truth[n].shape and bool(torch.isfinite(got[n]).all()), n
        for name, metric in (("peak", R.peak), ("l2", R.l2)):
            m, bar = metric(got[n], truth[n]), R.MARGIN * metric(own[n], truth[n])
            print(what, n, name, "measured %.3e  bar %.3e" % (m, bar))
            if not m <= bar:
                bad[(n, name)] = (m, bar)
    assert not bad, bad


@pytest.mark.parametrize("record", M.RECORDS)
@pytest.mark.parametrize("dtype_name,attention", ROUTES)
def test_forward_and_gradients(record, dtype_name, attention):
    dtype = R.DTYPES[dtype_name]
    got, _ = _run(record, dtype, attention)
    truth, own = M.reference(record, torch.float64), M.reference(record, dtype)
    # hidden_0 is the embedding lookup: exact in every dtype, its bar of zero holds
    _within(f"{record}/{dtype_name}/{attention}", got, truth, own, M.names_of(M.CONFIGS[record]))


@pytest.mark.parametrize("record", M.RECORDS)
def test_gradient_checkpointing_changes_no_bit(record):
    outs = []
    for ckpt in (False, True):
        got, model = _run(record, torch.float16, "hip", gradient_checkpointing=ckpt)
        assert model.gradient_checkpointing is ckpt
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        outs.append((got, grads))
    (a, ga), (b, gb) = outs
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["loss"], b["loss"])
    assert ga.keys() == gb.keys() and len(ga) == 2 + 3 * 7 * M.CONFIGS[record]["num_hidden_layers"]
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


@pytest.mark.parametrize("record", M.RECORDS)
def test_round_trip_into_the_packed_model(record):
    from onebit_amd.checkpoint import convert_train_state_dict
    from onebit_amd.llama import OneBitLlamaForCausalLM
    cfg = M.CONFIGS[record]
    ids, _ = M.make_batch(cfg, M.SEEDS[record])
    model = _model(record, torch.float16, "hip")
    model.load_state_dict({k: v.half() for k, v in M.make_params(cfg, M.SEEDS[record]).items()}, strict=True)
    model = model.to(DEV)
    packed = convert_train_state_dict(model.state_dict(), device=DEV)
    inf = OneBitLlamaForCausalLM(OneBitLlamaConfig(**cfg), torch.float16)
    inf.load_state_dict(packed, strict=True)
    inf = inf.to(DEV).eval()
    got = {"logits": inf(ids.to(DEV)).double().cpu()}
    _within(f"{record}/packed", got, M.reference(record, torch.float64), M.reference(record, torch.float16), ["logits"])


def test_hidden_states_feed_kdloss():
    from onebit_amd.kd import KDLoss
    record = "gqa"
    cfg = M.CONFIGS[record]
    ids, labels = M.make_batch(cfg, M.SEEDS[record])
    model = _model(record, torch.float16, "hip")
    model.load_state_dict({k: v.half() for k, v in M.make_params(cfg, M.SEEDS[record]).items()}, strict=True)
    model = model.to(DEV)
    logits, states, loss = model(ids.to(DEV), labels=labels.to(DEV), output_hidden_states=True)
    L = cfg["num_hidden_layers"]
    assert isinstance(states, tuple) and len(states) == L + 1 and logits.dtype == torch.float32 and loss is not None
    assert all(s.shape == (M.BATCH, M.SEQ, cfg["hidden_size"]) and s.dtype == torch.float16 for s in states)
    g = torch.Generator(device=DEV).manual_seed(11)
    t_logits = torch.randn(logits.shape, device=DEV, dtype=torch.float16, generator=g)
    t_states = tuple(torch.randn(s.shape, device=DEV, dtype=torch.float16, generator=g) for s in states)
    total = KDLoss(kd_alpha=0.8, kd_beta=0.1)(logits.half(), t_logits, labels.to(DEV), states, t_states)
    assert bool(torch.isfinite(total))
    total.backward()
    n_train = 0
    for k, p in model.named_parameters():
        if k.endswith("layernorm.weight") or k == "model.norm.weight":
            assert not p.requires_grad and p.grad is None, k
        elif p.requires_grad:
            n_train += 1
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            assert float(p.grad.abs().max()) > 0, k
    assert n_train == 3 * 7 * L
    # without labels and hidden states: logits alone
    with torch.no_grad():
        l2, s2, loss2 = model(ids.to(DEV))
    assert s2 is None and loss2 is None and torch.equal(l2, logits.detach())


def test_from_teacher_state_dict():
    from onebit_amd.train_model import OneBitLlamaForCausalLMTrain
    cfg = M.CONFIGS["gqa"]
    g = torch.Generator().manual_seed(21)
    Hd = cfg["hidden_size"]
    teacher = {"model.embed_tokens.weight": torch.randn(cfg["vocab_size"], Hd, generator=g).half(),
               "model.norm.weight": torch.ones(Hd).half(),
               "lm_head.weight": (0.05 * torch.randn(cfg["vocab_size"], Hd, generator=g)).half()}
    for l in range(cfg["num_hidden_layers"]):
        for name, K, N in M.proj_shapes(cfg):
            teacher[f"model.layers.{l}.{name}.weight"] = (0.05 * torch.randn(N, K, generator=g)).half()
        teacher[f"model.layers.{l}.input_layernorm.weight"] = torch.ones(Hd).half()
        teacher[f"model.layers.{l}.post_attention_layernorm.weight"] = torch.ones(Hd).half()
    model = OneBitLlamaForCausalLMTrain.from_teacher_state_dict(OneBitLlamaConfig(**cfg), teacher, device=DEV)
    q = model.model.layers[0].self_attn.q_proj
    assert q.weight.is_cuda and bool((q.weight.abs() == q.weight.abs().flatten()[0]).all())       # sign * 0.01
    assert torch.equal(model.lm_head.weight.cpu(), teacher["lm_head.weight"])
    ids, labels = M.make_batch(cfg, 3)
    logits, _, loss = model(ids.to(DEV), labels=labels.to(DEV))
    assert logits.shape == (M.BATCH, M.SEQ, cfg["vocab_size"]) and bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss))
    loss.backward()
    assert bool(torch.isfinite(q.weight.grad).all())
