"""Host restatement of the knowledge-distillation objective (onebit_amd/kd.py, include/onebit.h ``onebit_kd_*``) for the
tests: the torch op sequence of the reference's ``KDTrainer.ce_loss`` / ``compute_loss`` (``llamafactory/kd.py:34-113``) plus
the causal-LM cross-entropy its student model returns, evaluated in float64 on the CPU with torch autograd.

Pinned by ``tests/golden/kd_loss.npz`` (recorded from the reference's own functions, ``tests/golden/gen_goldens_kd.py``);
``tests/test_kd_cpu.py`` checks that this module reproduces the fixture to 1e-12.  Only tests (and the benchmark's torch
baseline, in the device's own dtype) import it; the product never does.
"""
import torch
import torch.nn.functional as F


def kl_batchmean(student_logits, teacher_logits):
    """``KDTrainer.ce_loss``: sum over ALL rows and entries, divided by the first dimension only."""
    return F.kl_div(F.log_softmax(student_logits, dim=2), F.softmax(teacher_logits, dim=2), reduction="batchmean")


def causal_ce(student_logits, labels, ignore_index=-100):
    """The student model's own loss: position s scored against labels[:, s + 1], mean over the labelled rows."""
    V = student_logits.shape[-1]
    shift_logits = student_logits[:, :-1, :].reshape(-1, V)
    shift_labels = labels[:, 1:].reshape(-1)
    return F.cross_entropy(shift_logits, shift_labels, ignore_index=ignore_index)


def token_loss(student_logits, teacher_logits, labels, kd_alpha, kd_loss_scale, ignore_index=-100):
    """(loss, kl, ce); kl is 0.0 when kd_loss_scale <= 0 (kd.py:71-74), the CE term is dropped when labels is None."""
    kl = kl_batchmean(student_logits, teacher_logits) if kd_loss_scale > 0.0 else 0.0
    loss = kd_alpha * kd_loss_scale * kl
    ce = None
    if labels is not None:
        ce = causal_ce(student_logits, labels, ignore_index)
        loss = loss + (1 - kd_alpha) * ce
    return loss, kl, ce


def hidden_pair(student_state, teacher_state):
    t = teacher_state.reshape(-1, teacher_state.shape[-1])
    s = student_state.reshape(-1, t.shape[-1])
    diff = F.normalize(t, p=2, dim=1) - F.normalize(s, p=2, dim=1)
    return torch.mean(torch.norm(diff, p=2, dim=1) ** 2)


def hidden_loss(student_states, teacher_states):
    total = 0.0
    for s, t in zip(student_states, teacher_states):
        total = total + hidden_pair(s, t)
    return total


def kd_loss(student_logits, teacher_logits, labels, student_states=None, teacher_states=None, n_layers=None,
            kd_alpha=0.8, kd_beta=0.0, kd_loss_scale=1.0, ignore_index=-100):
    """``compute_loss`` with kd_gamma = 0: the hidden term over entries 0 .. n_layers - 1 of the state tuples."""
    loss, _, _ = token_loss(student_logits, teacher_logits, labels, kd_alpha, kd_loss_scale, ignore_index)
    if kd_beta > 0:
        n = len(student_states) - 1 if n_layers is None else n_layers
        loss = loss + kd_beta * hidden_loss(student_states[:n], teacher_states[:n])
    return loss


def to64(x):
    """A CPU float64 leaf copy of a tensor (values exactly those of its fp16 / fp32 original)."""
    return x.detach().to("cpu", torch.float64).requires_grad_(True)
