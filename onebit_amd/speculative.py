"""Speculative decoding with prompt-lookup drafts: the host statement of what ``ob_spec_commit_kernel`` (csrc/ob_spec.h) does on
the device at the end of every speculative step -- its documentation, and the drafter for callers without the native step.

A step verifies ``k`` draft tokens behind the sequence's last token in ONE pass over the weights (``engine.SpecStep``):
``chosen[i]`` is the token the model emits after row ``i`` (argmax, or the sampler's draw -- a pure function of the row's logits,
the request's parameters and the position).  The drafts ``chosen`` confirms are emitted together with the one token that follows
them, so the output is exactly what one-token-at-a-time decoding through the same step emits; a draft only decides how many
tokens a step yields.  No draft model: the drafts are the tokens that followed the most recent earlier occurrence of the
sequence's last n-gram in its own history."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple


@dataclass(frozen=True)
class SpecConfig:
    """``draft_tokens``: drafts verified per step (1 .. 15; a step runs ``draft_tokens + 1`` token rows).  ``ngram_max`` /
    ``ngram_min``: the longest / shortest suffix n-gram looked up in the history (1 <= min <= max <= 16)."""
    draft_tokens: int
    ngram_max: int = 3
    ngram_min: int = 1

    def __post_init__(self):
        if not 1 <= int(self.draft_tokens) <= 15:
            raise ValueError("SpecConfig: draft_tokens must be in 1..15")
        if not 1 <= int(self.ngram_min) <= int(self.ngram_max) <= 16:
            raise ValueError("SpecConfig: need 1 <= ngram_min <= ngram_max <= 16")


def propose(history: Sequence[int], k: int, ngram_max: int = 3, ngram_min: int = 1) -> Tuple[List[int], int]:
    """``k`` draft tokens for the sequence ``history`` (its last token included) and how many of them came from a match.
    For n = ngram_max down to ngram_min: the LATEST earlier occurrence of the last n tokens (it may overlap the suffix, it ends
    before the last token, so at least one token follows it); the first n that has one supplies up to ``k`` followers.  The
    remaining slots repeat the last token."""
    h = list(history)
    P = len(h) - 1
    for n in range(min(ngram_max, P), ngram_min - 1, -1):
        for e in range(P - 1, n - 2, -1):                      # the match ends at e: latest first
            if h[e - n + 1:e + 1] == h[P - n + 1:P + 1]:
                got = h[e + 1:min(e + k, P) + 1]
                return got + [h[P]] * (k - len(got)), len(got)
    return [h[P]] * k, 0


def accept(drafts: Sequence[int], chosen: Sequence[int]) -> int:
    """Number of accepted drafts: the longest prefix with ``drafts[i] == chosen[i]`` (``chosen`` has one entry more than
    ``drafts``; the step emits ``chosen[:n + 1]``)."""
    n = 0
    while n < len(drafts) and drafts[n] == chosen[n]:
        n += 1
    return n
