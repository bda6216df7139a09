"""numpy restatement of the speculative step's commit contract (accept the verified draft prefix, append, draft the next step
by prompt lookup), written from the feature's specification -- not from the kernel or from onebit_amd/speculative.py:

  n_acc     the longest prefix with draft[i] == chosen[i], capped so that pos + n_acc + 1 < max_len and by the `remaining` budget
            (n_acc + 1 tokens are emitted; when the caps leave no room for even one token nothing is emitted and n_acc = -1)
  history   the n_acc + 1 emitted tokens chosen[0 .. n_acc] follow position pos; pos and remaining advance by n_acc + 1
  drafts    the longest suffix n-gram, n from ngram_max down to ngram_min, with an earlier occurrence (one that ends before the
            last token, so at least one token follows it; it may overlap the suffix); the MOST RECENT such occurrence; up to k
            of the tokens that follow it; the remaining draft slots repeat the sequence's last token
  next step tokens = [last token, drafts], row_pos = pos .. pos + k, record = (n_acc, pos, n_drafted)
"""
import numpy as np


def propose_ref(history, k, ngram_max, ngram_min):
    h = np.asarray(history, dtype=np.int64)
    last = len(h) - 1
    for n in range(ngram_max, ngram_min - 1, -1):
        if n > last:                       # an earlier occurrence needs n tokens that end before the last one
            continue
        suffix = h[last - n + 1:]
        starts = [s for s in range(0, last - n + 1) if np.array_equal(h[s:s + n], suffix)]     # s + n - 1 <= last - 1
        if starts:
            f0 = max(starts) + n           # first follower of the most recent occurrence
            got = [int(t) for t in h[f0:f0 + k]]
            return got + [int(h[last])] * (k - len(got)), len(got)
    return [int(h[last])] * k, 0


def accept_ref(drafts, chosen):
    n = 0
    for d, c in zip(drafts, chosen):
        if d != c:
            break
        n += 1
    return n


def commit_ref(chosen, drafts, pos, remaining, history, max_len, ngram_max, ngram_min):
    """-> dict(n_acc, pos, remaining, n_drafted, history (new, a list of pos + 1 tokens), tokens, row_pos, drafts)"""
    k = len(drafts)
    assert len(chosen) == k + 1 and len(history) == pos + 1
    n_emit = accept_ref(drafts, chosen) + 1
    while n_emit > 0 and not (pos + n_emit < max_len and n_emit <= remaining):
        n_emit -= 1
    hist = [int(t) for t in history] + [int(t) for t in chosen[:n_emit]]
    new_pos = pos + n_emit
    nd, n_drafted = propose_ref(hist, k, ngram_max, ngram_min)
    return dict(n_acc=n_emit - 1, pos=new_pos, remaining=remaining - n_emit, n_drafted=n_drafted, history=hist,
                tokens=[hist[-1]] + nd, row_pos=list(range(new_pos, new_pos + k + 1)), drafts=nd)
