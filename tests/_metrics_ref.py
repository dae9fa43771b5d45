"""Evaluation counters restated in numpy: what dk_classify_accumulate_f32
(dorknet_amd/csrc/metrics.hip) computes, and what it is measured against.

Per row b with label y and scores s (fp32):

- pred = np.argmax(s): of equal maxima the lowest index (FeedForwardNetwork.test's rule).
- rank = #{j : s[j] > s[y]} + #{j > y : s[j] == s[y]}: the position of y in
  np.argsort(s, kind="stable")[::-1], so rank < k exactly when y is in tests/_cam_ref.topk_rows(s, k).
- nll = -log(s[y]): fp64 here; the kernel's is -logf(s[y]) in fp32, held to it within
  1e-5 * max(1, |nll|) (the bound of tests/test_gpu_layers.py for this logf).
- a label outside [0, classes): the row is ignored; state[1] += 1 and nothing else; rank = -1, nll = 0,
  pred still written.
- a row whose nll is not finite: state[3] += 1, nothing added to state[4]; counted everywhere else.
- NaN scores: pred and rank are unspecified but inside [0, classes).  This restatement takes the kernel's
  reading for a row that holds finite scores besides the NaNs (a NaN compares false to everything, so it
  never wins the maximum and counts in no rank); np.argmax would return the NaN's index.

state (int64, 22 words): [0] n counted, [1] ignored, [2] pred == y, [3] non-finite, [4] sum of
rint(nll * 2^32) over the finite rows (Q32), [5 + r] rank == r for r < 16, [21] rank >= 16.
confusion[y][pred] += 1 per counted row.

The Q32 word depends on the fp32 nll values, which come from the device's logf; ``q32_sum`` forms it
from given fp32 values, and ``accumulate`` fills state[4] from its own fp64 nll rounded to fp32 (what
an exactly rounded logf would give), which a GPU test replaces by q32_sum of the kernel's nll_out.
"""
import numpy as np

STATE_WORDS = 22
RANK_BINS = 16
Q32 = 2.0 ** 32


def q32_sum(nll32):
    """sum of rint((double)nll * 2^32) over the finite entries of fp32 values, as a Python int."""
    a = np.asarray(nll32, dtype=np.float32).astype(np.float64)
    a = a[np.isfinite(a)]
    return int(sum(int(v) for v in np.rint(a * Q32)))


def rank_of(s, y):
    s = np.asarray(s)
    with np.errstate(invalid="ignore"):
        return int(np.sum(s > s[y]) + np.sum(s[y + 1:] == s[y]))


def accumulate(scores, labels, classes):
    """scores (N, classes) fp32, labels (N,) integers -> (state int64 (22,), confusion int64
    (classes, classes), pred int32 (N,), rank int32 (N,), nll64 float64 (N,))."""
    scores = np.asarray(scores, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    N = scores.shape[0]
    assert scores.shape == (N, classes) and labels.shape == (N,)
    state = np.zeros(STATE_WORDS, dtype=np.int64)
    confusion = np.zeros((classes, classes), dtype=np.int64)
    pred = np.zeros(N, dtype=np.int32)
    rank = np.zeros(N, dtype=np.int32)
    nll = np.zeros(N, dtype=np.float64)
    q = 0
    for b in range(N):
        s, y = scores[b], int(labels[b])
        pred[b] = np.argmax(np.where(np.isnan(s), -np.inf, s))
        if not 0 <= y < classes:
            state[1] += 1
            rank[b] = -1
            continue
        rank[b] = rank_of(s, y)
        with np.errstate(divide="ignore", invalid="ignore"):
            nll[b] = -np.log(np.float64(s[y]))
        state[0] += 1
        state[2] += int(pred[b] == y)
        if np.isfinite(nll[b]):
            q += int(np.rint(np.float64(np.float32(nll[b])) * Q32))
        else:
            state[3] += 1
        state[5 + min(int(rank[b]), RANK_BINS)] += 1
        confusion[y, pred[b]] += 1
    state[4] = q
    return state, confusion, pred, rank, nll
