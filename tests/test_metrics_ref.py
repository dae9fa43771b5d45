"""Evaluation counters without a GPU: the numpy restatement of tests/_metrics_ref.py
pinned against np.argsort / np.argmax / tests/_cam_ref.topk_rows and known answers, the Q32 fixed-point
facts the loss word rests on, the argument checks of ClassificationMeter.update, FeedForwardNetwork.evaluate
and .predict, and the C entry points' refusal of bad arguments (no launch)."""
import os

import numpy as np
import pytest

from tests import _cam_ref as cam_ref
from tests import _metrics_ref as ref

from dorknet_amd import _hip
from dorknet_amd.metrics import ClassificationMeter, ClassificationReport


def _tie_heavy(rows=200, classes=23, seed=11):
    rng = np.random.RandomState(seed)
    scores = rng.randint(0, 4, size=(rows, classes)).astype(np.float32)   # values in {0, 1, 2, 3}: ties everywhere
    labels = rng.randint(0, classes, size=rows)
    return scores, labels


def test_rank_is_the_position_in_the_reversed_stable_argsort():
    scores, labels = _tie_heavy()
    _, _, _, rank, _ = ref.accumulate(scores, labels, scores.shape[1])
    for s, y, r in zip(scores, labels, rank):
        order = np.argsort(s, kind="stable")[::-1]
        assert order[r] == y


def test_rank_below_k_is_membership_in_topk_rows():
    scores, labels = _tie_heavy()
    _, _, _, rank, _ = ref.accumulate(scores, labels, scores.shape[1])
    for k in (1, 3, 16):
        top = cam_ref.topk_rows(scores, k)
        member = (top == labels[:, None]).any(axis=1)
        assert np.array_equal(rank < k, member)


def test_pred_is_argmax_lowest_index_first():
    scores, labels = _tie_heavy()
    state, confusion, pred, _, _ = ref.accumulate(scores, labels, scores.shape[1])
    assert np.array_equal(pred, np.argmax(scores, axis=1))
    assert state[2] == np.sum(pred == labels) and state[0] == len(labels)
    assert confusion.sum() == len(labels)
    assert np.array_equal(confusion.sum(axis=1), np.bincount(labels, minlength=scores.shape[1]))
    # the two tie rules differ somewhere on such rows, and only where the maximum is tied
    _, _, _, rank, _ = ref.accumulate(scores, labels, scores.shape[1])
    differ = (pred == labels) != (rank == 0)
    assert differ.any()
    for s in scores[differ]:
        assert np.sum(s == s.max()) > 1


def test_known_answers():
    classes = 7
    for y in range(classes):
        state, confusion, pred, rank, nll = ref.accumulate(np.full((1, classes), 0.25, np.float32), [y], classes)
        assert pred[0] == 0 and rank[0] == classes - 1 - y
        assert confusion[y, 0] == 1 and confusion.sum() == 1
        assert state[2] == int(y == 0) and state[5 + classes - 1 - y] == 1
        assert nll[0] == -np.log(0.25)
    # two classes
    s = np.array([[0.75, 0.25], [0.25, 0.75], [0.5, 0.5]], np.float32)
    state, confusion, pred, rank, nll = ref.accumulate(s, [0, 0, 1], 2)
    assert pred.tolist() == [0, 1, 0] and rank.tolist() == [0, 1, 0]
    assert state[:4].tolist() == [3, 0, 1, 0] and state[5:7].tolist() == [2, 1] and not state[7:].any()
    assert confusion.tolist() == [[1, 1], [1, 0]]
    assert np.allclose(nll, -np.log([0.75, 0.25, 0.5]), rtol=0, atol=0)
    assert state[4] == ref.q32_sum(np.float32(nll))
    # a rank past the histogram's 16 bins
    s = np.arange(40, dtype=np.float32)[None]
    state, _, _, rank, _ = ref.accumulate(s, [3], 40)
    assert rank[0] == 36 and state[21] == 1 and not state[5:21].any()


def test_ignored_and_nonfinite_rows():
    classes = 5
    s = np.tile(np.array([0.1, 0.2, 0.4, 0.2, 0.1], np.float32), (5, 1))
    s[3, 1] = 0.0           # s[y] = 0: nll = +inf
    s[4, 4] = np.nan        # s[y] = NaN
    labels = [-1, classes, 2, 1, 4]
    state, confusion, pred, rank, nll = ref.accumulate(s, labels, classes)
    assert state[:4].tolist() == [3, 2, 1, 2]
    assert rank[:2].tolist() == [-1, -1] and nll[:2].tolist() == [0, 0] and pred[:2].tolist() == [2, 2]
    assert state[4] == ref.q32_sum([np.float32(-np.log(np.float64(np.float32(0.4))))])
    assert confusion.sum() == 3 and confusion[2, 2] == 1 and confusion[1, 2] == 1 and confusion[4, 2] == 1
    assert state[5:].sum() == 3


def test_q32_facts():
    rng = np.random.RandomState(5)
    # an fp32 value >= 2^-9 has an ulp >= 2^-32: times 2^32 it is an integer, carried exactly
    v = np.concatenate([rng.uniform(2.0 ** -9, 104, 5000), [2.0 ** -9, 103.27893]]).astype(np.float32)
    v = v[v >= np.float32(2.0 ** -9)].astype(np.float64)
    assert np.array_equal(np.rint(v * ref.Q32), v * ref.Q32)
    # below that a row is off by at most half a unit of 2^-32
    w = rng.uniform(0, 2.0 ** -9, 5000).astype(np.float32).astype(np.float64)
    assert np.max(np.abs(np.rint(w * ref.Q32) / ref.Q32 - w)) <= 2.0 ** -33
    # capacity: the worst finite fp32 case is s[y] = 2^-149, nll = 103.28; about 2.0e7 such rows fit int64
    worst = np.float32(-np.log(2.0 ** -149))
    assert 103.2 < worst < 103.3
    rows = 2 ** 63 / (float(worst) * ref.Q32)
    assert 2.0e7 < rows < 2.1e7
    assert 2 ** 63 / (5 * ref.Q32) > 4e8
    # the report's loss is the mean of the fp32 values when they are exact in Q32
    nll = np.array([0.5, 1.25, 3.0], np.float32)
    state = np.zeros(ref.STATE_WORDS, np.int64)
    state[0], state[3], state[4] = 4, 1, ref.q32_sum(nll)
    assert ClassificationReport(state).loss == float(np.mean(nll.astype(np.float64)))


def test_report_fields():
    scores, labels = _tie_heavy(rows=50, classes=20)
    state, confusion, pred, rank, _ = ref.accumulate(scores + 1, labels, 20)
    rep = ClassificationReport(state, confusion, top=(1, 5))
    assert rep.n == 50 and rep.ignored == 0 and rep.nonfinite == 0 and rep.correct == int(np.sum(pred == labels))
    assert rep.accuracy == rep.correct / 50
    assert rep.rank_hist.shape == (17,) and rep.rank_hist.dtype == np.int64 and rep.rank_hist.sum() == 50
    for k in (1, 5, 16):
        assert rep.top_k(k) == np.sum(rank < k) / 50
    for k in (0, 17):
        with pytest.raises(ValueError):
            rep.top_k(k)
    per = rep.per_class_accuracy
    seen = np.bincount(labels, minlength=20) > 0
    assert np.array_equal(np.isnan(per), ~seen)
    assert np.allclose(per[seen], (np.diag(confusion) / np.maximum(confusion.sum(axis=1), 1))[seen], rtol=0, atol=0)
    empty = ClassificationReport(np.zeros(ref.STATE_WORDS, np.int64))
    assert np.isnan(empty.loss) and np.isnan(empty.accuracy) and empty.confusion is None
    assert empty.per_class_accuracy is None
    assert "top-5" in repr(rep)


def test_meter_argument_errors_need_no_gpu():
    import torch
    with pytest.raises(ValueError):
        ClassificationMeter(1)
    m = ClassificationMeter(5)
    ok = torch.zeros((3, 5))
    bad = [
        (torch.zeros(5), [0]),                                  # wrong rank
        (torch.zeros((3, 5, 1)), [0, 1, 2]),
        (ok, [0, 1]),                                           # row count differs from the labels'
        (ok, torch.zeros(4, dtype=torch.int64)),
        (ok.double(), [0, 1, 2]),                               # not fp32
        (ok.to(torch.bfloat16), [0, 1, 2]),
        (torch.zeros((3, 6)), [0, 1, 2]),                       # classes do not match
        (ok, [0.0, 1.0, 2.0]),                                  # labels are no integers
        (ok, torch.zeros(3)),
        (ok, [[0, 1, 2]]),
        (ok.numpy(), [0, 1, 2]),                                # not a tensor
    ]
    for scores, labels in bad:
        with pytest.raises(ValueError):
            m.update(scores, labels)
    with pytest.raises(ValueError):
        m.merge(ClassificationMeter(6))
    with pytest.raises(ValueError):
        m.merge(ClassificationMeter(5, confusion=True))
    rep = m.result()      # nothing was added and nothing was allocated
    assert rep.n == 0 and rep.confusion is None and np.isnan(rep.loss)
    assert ClassificationMeter(3, confusion=True).result().confusion.shape == (3, 3)


def test_network_argument_errors_need_no_gpu():
    from examples.resnet18_depsep import ResNet18

    class Loader:
        def __iter__(self):
            raise AssertionError("the loader must not be touched before the arguments are checked")

    net = ResNet18("args")
    for top in ((0,), (1, 17), (), 0, ("a",)):
        with pytest.raises(ValueError):
            net.evaluate(Loader(), top=top)
    with pytest.raises(ValueError):
        net.evaluate(Loader(), num_batches=0)
    with pytest.raises(ValueError, match="no batch"):
        net.evaluate([])
    X = np.zeros((2, 3, 65, 65), np.float32)
    for top in (0, 17, 2.5, None):
        with pytest.raises(ValueError):
            net.predict(X, top=top)
    with pytest.raises(ValueError):
        net.predict(np.zeros(3, np.float32))


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")
def test_entry_points_refuse_bad_arguments_without_a_launch():
    lib = _hip.lib
    p = 256   # stands for a device pointer: nothing is launched, so nothing reads it

    def classify(scores=p, labels=p, N=4, classes=5, state=p):
        lib.dk_classify_accumulate_f32(scores, labels, N, classes, state, p, p, p, p, None)

    for kw in (dict(N=0), dict(N=-3), dict(classes=1), dict(classes=0), dict(scores=0), dict(labels=0), dict(state=0),
               dict(classes=2 ** 31 - 1)):
        with pytest.raises(_hip.HipError, match="10001"):
            classify(**kw)
    for N, classes, K, idx, val in ((0, 5, 1, p, p), (1, 0, 1, p, p), (1, 5, 0, p, p), (1, 5, 6, p, p),
                                    (1, 40, 17, p, p), (1, 5, 2, 0, p), (1, 5, 2, p, 0)):
        with pytest.raises(_hip.HipError, match="10001"):
            lib.dk_topk_rows_vals_f32(p, N, classes, K, idx, val, None)
    assert "dk_classify_accumulate_f32" in lib.declarations and "dk_topk_rows_vals_f32" in lib.declarations
