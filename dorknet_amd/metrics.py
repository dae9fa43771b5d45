"""Evaluation on the GPU: accuracy, top-k, confusion matrix and loss.

Reference: ``FeedForwardNetwork.test`` (network/feed_forward_network.py:72-80) copies every batch's
(N, classes) scores to the host and compares there; examples/imagenet_dogs_225_resnet_18_depsep_evaluate.py
arg-sorts one image's scores for its best five.  Here one HIP launch per batch
(dk_classify_accumulate_f32, dorknet_amd/csrc/metrics.hip) adds everything to device-resident int64
counters, and the host reads them once:

- ``ClassificationMeter(classes, confusion=False)``: ``update(scores, labels, want_rows=False)`` (one
  launch, no synchronisation), ``reset()``, ``merge(other)``, ``result()`` (the only call that
  synchronises) -> ``ClassificationReport``.
- ``ClassificationReport``: ``n``, ``ignored``, ``nonfinite``, ``correct``, ``rank_hist``, ``accuracy``,
  ``top_k(k)``, ``loss``, ``confusion``, ``per_class_accuracy``.
- ``FeedForwardNetwork.evaluate`` and ``.predict`` run the network and call these.

Two tie rules, both the reference's: ``correct`` counts ``np.argmax`` (of equal maxima the lowest index,
as ``test`` does), the rank histogram follows ``np.argsort(scores)[::-1]`` (of equal scores the higher
index first, as the evaluate program and ``top_classes`` do).  ``accuracy`` and ``top_k(1)`` differ only
on rows whose maximum is tied.  A label outside [0, classes) makes its row ignored (padding).
"""
from __future__ import annotations

import numpy as np
import torch

from ._hip import lib, stream_handle
from ._tensor import F32, device

STATE_WORDS = 22     # DK_CLASSIFY_STATE_WORDS
RANK_BINS = 16       # rank_hist[r], r < 16: rows with rank r; rank_hist[16]: rank >= 16
_Q32 = 2.0 ** -32


class ClassificationReport:
    """The counters of a ClassificationMeter on the host.  state: int64 (22,); confusion: int64
    (classes, classes) or None."""

    def __init__(self, state, confusion=None, top=(1,)):
        state = np.asarray(state, dtype=np.int64).reshape(STATE_WORDS)
        self.state = state
        self.n = int(state[0])
        self.ignored = int(state[1])
        self.correct = int(state[2])
        self.nonfinite = int(state[3])
        self.rank_hist = state[5:5 + RANK_BINS + 1].copy()
        self.confusion = None if confusion is None else np.asarray(confusion, dtype=np.int64)
        self.top = tuple(top)

    @property
    def accuracy(self):
        """Rows whose np.argmax is the label, over the rows counted."""
        return self.correct / self.n if self.n else float("nan")

    def top_k(self, k):
        """Rows whose label is among the k best classes (np.argsort(scores)[::-1][:k]), 1 <= k <= 16."""
        k = int(k)
        if not 1 <= k <= RANK_BINS:
            raise ValueError("top_k needs 1 <= k <= {}, got {}".format(RANK_BINS, k))
        return int(self.rank_hist[:k].sum()) / self.n if self.n else float("nan")

    @property
    def loss(self):
        """Mean of -log(score of the label) over the rows where it is finite (fp64, from the Q32 sum)."""
        m = self.n - self.nonfinite
        return int(self.state[4]) * _Q32 / m if m else float("nan")

    @property
    def per_class_accuracy(self):
        """The confusion matrix's diagonal over its row sums; NaN for a class with no rows."""
        if self.confusion is None:
            return None
        rows = self.confusion.sum(axis=1).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(rows > 0, np.diag(self.confusion) / rows, np.nan)

    def __repr__(self):
        tops = ", ".join("top-{} {:.4f}".format(k, self.top_k(k)) for k in self.top)
        return "ClassificationReport(n={}, ignored={}, nonfinite={}, accuracy {:.4f}, {}, loss {:.5f})".format(
            self.n, self.ignored, self.nonfinite, self.accuracy, tops, self.loss)


def _check_scores(scores, classes):
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
        raise ValueError("scores must be a 2-D (N, classes) tensor, got {}".format(
            tuple(scores.shape) if hasattr(scores, "shape") else type(scores)))
    if scores.dtype != F32:
        raise ValueError("scores must be fp32, got {}".format(scores.dtype))
    if scores.shape[0] < 1 or scores.shape[1] != classes:
        raise ValueError("scores must be (N >= 1, {}), got {}".format(classes, tuple(scores.shape)))


def _labels_int32(labels, n, classes):
    """Labels (a device or host tensor, a numpy array or a list) as a device int32 [n]; a value that
    int32 cannot hold becomes -1 (it is outside [0, classes) either way)."""
    if isinstance(labels, torch.Tensor):
        if labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise ValueError("labels must be a 1-D integer tensor, got {} {}".format(labels.dtype, tuple(labels.shape)))
        if labels.shape[0] != n:
            raise ValueError("{} labels for {} rows of scores".format(labels.shape[0], n))
        if labels.dtype != torch.int32:
            labels = labels.clamp(-1, classes)
        return labels.to(device=device(), dtype=torch.int32).contiguous()
    a = np.asarray(labels)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError("labels must be a 1-D sequence of integers, got {} {}".format(a.dtype, a.shape))
    if a.shape[0] != n:
        raise ValueError("{} labels for {} rows of scores".format(a.shape[0], n))
    a = np.where((a < 0) | (a >= classes), -1, a).astype(np.int32)
    # through pinned memory and without blocking: a copy from pageable memory waits for the stream,
    # i.e. for the forward pass that produced the scores
    return torch.from_numpy(a).pin_memory().to(device=device(), non_blocking=True)


class ClassificationMeter:
    """Device-resident evaluation counters for a `classes`-way classifier; confusion=True also keeps the
    int64 (classes, classes) matrix, rows the label, columns the prediction."""

    def __init__(self, classes, confusion=False):
        classes = int(classes)
        if classes < 2:
            raise ValueError("ClassificationMeter needs classes >= 2, got {}".format(classes))
        self.classes = classes
        self.with_confusion = bool(confusion)
        self._state = None       # allocated by the first update (a meter can be made without a GPU)
        self._confusion = None

    def _buffers(self):
        if self._state is None:
            self._state = torch.zeros(STATE_WORDS, dtype=torch.int64, device=device())
            if self.with_confusion:
                self._confusion = torch.zeros((self.classes, self.classes), dtype=torch.int64, device=device())
        return self._state, self._confusion

    def update(self, scores, labels, want_rows=False):
        """Add a batch: scores fp32 (N, classes), labels N integers.  One launch, no synchronisation.
        want_rows=True returns (pred int32, rank int32, nll fp32), each (N,) on the device."""
        _check_scores(scores, self.classes)
        n = scores.shape[0]
        y = _labels_int32(labels, n, self.classes)
        s = scores.to(device=device()).contiguous()
        state, conf = self._buffers()
        pred = rank = nll = None
        if want_rows:
            pred = torch.empty(n, dtype=torch.int32, device=s.device)
            rank = torch.empty(n, dtype=torch.int32, device=s.device)
            nll = torch.empty(n, dtype=F32, device=s.device)
        lib.dk_classify_accumulate_f32(s.data_ptr(), y.data_ptr(), n, self.classes, state.data_ptr(),
                                       0 if conf is None else conf.data_ptr(),
                                       0 if pred is None else pred.data_ptr(), 0 if rank is None else rank.data_ptr(),
                                       0 if nll is None else nll.data_ptr(), stream_handle())
        return (pred, rank, nll) if want_rows else None

    def reset(self):
        if self._state is not None:
            self._state.zero_()
            if self._confusion is not None:
                self._confusion.zero_()

    def merge(self, other):
        """Add another meter's counters to this one's (an integer vector add)."""
        if not isinstance(other, ClassificationMeter) or other.classes != self.classes \
                or other.with_confusion != self.with_confusion:
            raise ValueError("merge needs a ClassificationMeter of the same classes and confusion setting")
        if other._state is None:
            return
        state, conf = self._buffers()
        state += other._state
        if conf is not None:
            conf += other._confusion

    def result(self, top=(1,)):
        """The counters on the host: the one call that synchronises."""
        if self._state is None:
            conf = np.zeros((self.classes, self.classes), dtype=np.int64) if self.with_confusion else None
            return ClassificationReport(np.zeros(STATE_WORDS, dtype=np.int64), conf, top)
        conf = None if self._confusion is None else self._confusion.cpu().numpy()
        return ClassificationReport(self._state.cpu().numpy(), conf, top)
