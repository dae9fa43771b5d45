"""Evaluation counters on the GPU: dk_classify_accumulate_f32 against the restatement
of tests/_metrics_ref.py -- the integer words, the confusion matrix, pred and rank with np.array_equal, the
per-row nll within the project's bound for this logf, the Q32 loss word exactly from the kernel's own nll
values -- ClassificationMeter, dk_topk_rows_vals_f32 / predict, and FeedForwardNetwork.evaluate."""
import functools

import numpy as np
import pytest

from tests import _cam_ref as cam_ref
from tests import _metrics_ref as ref

from dorknet_amd.cam import top_classes, top_classes_with_scores
from dorknet_amd.metrics import ClassificationMeter

# (N, classes): one row of two classes; fewer classes than lanes; the model's head (float4 rows); scalar
# columns with N no multiple of the four waves of a workgroup; more than 256 rows; several loads per lane
# (inside the 1024 columns a wave keeps in registers); a row past them (read again for the rank)
SHAPES = [(1, 2), (5, 5), (3, 120), (67, 121), (260, 120), (2, 1000), (3, 4100)]


@functools.lru_cache(maxsize=None)
def _case(N, classes):
    """Softmax probabilities and labels of a shape, drawn once from a fixed seed, with their restatement."""
    rng = np.random.RandomState(1000 * N + classes)
    z = 2.0 * rng.standard_normal((N, classes))
    e = np.exp(z)
    scores = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    labels = rng.randint(0, classes, size=N).astype(np.int32)
    labels[0] = int(np.argmax(scores[0]))      # at least one correct row
    want = ref.accumulate(scores, labels, classes)
    for a in (scores, labels) + want:
        a.setflags(write=False)
    return scores, labels, want


def _run(scores, labels, state=None, confusion=True, rows=True):
    """The C entry point on device copies; the row outputs pre-filled so an unwritten element shows."""
    import torch
    from dorknet_amd._hip import lib, stream_handle
    N, classes = scores.shape
    s = torch.from_numpy(np.array(scores, dtype=np.float32)).cuda()
    y = torch.from_numpy(np.array(labels, dtype=np.int32)).cuda()
    st = torch.zeros(ref.STATE_WORDS, dtype=torch.int64, device="cuda") if state is None else state
    cf = torch.zeros((classes, classes), dtype=torch.int64, device="cuda") if confusion else None
    pred = torch.full((N,), -7, dtype=torch.int32, device="cuda") if rows else None
    rank = torch.full((N,), -7, dtype=torch.int32, device="cuda") if rows else None
    nll = torch.full((N,), 77.0, dtype=torch.float32, device="cuda") if rows else None
    lib.dk_classify_accumulate_f32(s.data_ptr(), y.data_ptr(), N, classes, st.data_ptr(),
                                   0 if cf is None else cf.data_ptr(), 0 if pred is None else pred.data_ptr(),
                                   0 if rank is None else rank.data_ptr(), 0 if nll is None else nll.data_ptr(),
                                   stream_handle())
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(st), host(cf), host(pred), host(rank), host(nll)


def _check(got, want, labels, classes):
    state, confusion, pred, rank, nll = got
    wstate, wconf, wpred, wrank, wnll = want
    assert np.array_equal(state[:4], wstate[:4]), (state, wstate)
    assert np.array_equal(state[5:], wstate[5:]), (state, wstate)
    assert np.array_equal(confusion, wconf)
    assert np.array_equal(pred, wpred) and np.array_equal(rank, wrank)
    assert pred.min() >= 0 and pred.max() < classes and rank.max() < classes
    counted = (np.asarray(labels) >= 0) & (np.asarray(labels) < classes)
    fin = counted & np.isfinite(wnll)
    err = np.abs(nll[fin].astype(np.float64) - wnll[fin])
    bound = 1e-5 * np.maximum(1.0, np.abs(wnll[fin]))
    print("nll: worst error / bound {:.3g}".format(float(np.max(err / bound)) if err.size else 0.0))
    assert np.all(err <= bound)
    assert not nll[~counted].any()
    assert int(state[4]) == ref.q32_sum(nll[fin]), (int(state[4]), ref.q32_sum(nll[fin]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_classify_accumulate(shape):
    scores, labels, want = _case(*shape)
    _check(_run(scores, labels), want, labels, shape[1])


@pytest.mark.gpu
def test_unaligned_rows_take_the_scalar_path():
    """classes % 4 == 0 but a base pointer that is not 16-byte aligned: no float4 loads."""
    import torch
    from dorknet_amd._hip import lib, stream_handle
    scores, labels, want = _case(3, 120)
    buf = torch.zeros(3 * 120 + 1, dtype=torch.float32, device="cuda")
    s = buf[1:].view(3, 120)
    s.copy_(torch.from_numpy(np.array(scores)))
    assert s.data_ptr() % 16 == 4
    y = torch.from_numpy(np.array(labels)).cuda()
    st = torch.zeros(ref.STATE_WORDS, dtype=torch.int64, device="cuda")
    rank = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    lib.dk_classify_accumulate_f32(s.data_ptr(), y.data_ptr(), 3, 120, st.data_ptr(), 0, 0, rank.data_ptr(), 0,
                                   stream_handle())
    assert np.array_equal(rank.cpu().numpy(), want[3])
    assert np.array_equal(st.cpu().numpy()[:4], want[0][:4]) and np.array_equal(st.cpu().numpy()[5:], want[0][5:])


@pytest.mark.gpu
def test_ties():
    import torch
    rng = np.random.RandomState(3)
    N, classes = 40, 23
    scores = rng.randint(0, 4, size=(N, classes)).astype(np.float32)
    labels = rng.randint(0, classes, size=N).astype(np.int32)
    for b in range(0, 10):                       # the label on the tied maximum
        labels[b] = np.flatnonzero(scores[b] == scores[b].max())[-1]
    for b in range(10, 20):                      # and off it
        labels[b] = np.flatnonzero(scores[b] != scores[b].max())[0]
    scores[39, :] = 2.0                          # one all-equal row
    labels[39] = 7
    want = ref.accumulate(scores, labels, classes)
    got = _run(scores, labels)
    _check(got, want, labels, classes)
    _, _, pred, rank, _ = got
    # the pred rule: np.argmax, the lowest index of equal maxima
    assert np.array_equal(pred, np.argmax(scores, axis=1))
    assert pred[39] == 0 and rank[39] == classes - 1 - 7
    # the rank rule: the position in the reversed stable arg-sort; rank < k is membership in top_classes
    for b in range(N):
        assert np.argsort(scores[b], kind="stable")[::-1][rank[b]] == labels[b]
    multi = np.array([np.sum(s == s.max()) > 1 for s in scores[:10]])
    assert multi.any() and ((pred[:10] == labels[:10]) != (rank[:10] == 0))[multi].all()
    for k in (1, 3, 16):
        top = top_classes(torch.from_numpy(scores), k).cpu().numpy()
        assert np.array_equal(top, cam_ref.topk_rows(scores, k))
        assert np.array_equal(rank < k, (top == labels[:, None]).any(axis=1))


@pytest.mark.gpu
def test_ignored_and_nonfinite_rows():
    classes = 6
    scores = np.array(_case(67, 121)[0][:8, :classes])
    labels = np.array([-1, classes, 2, 1, 4, 0, 2 ** 31 - 1, 3], dtype=np.int32)
    scores[3, 1] = 0.0            # s[y] = 0
    scores[4, 4] = np.nan         # s[y] = NaN (the row's other scores are finite)
    want = ref.accumulate(scores, labels, classes)
    assert want[0][:4].tolist() == [5, 3, int(np.sum(want[2][[2, 3, 4, 5, 7]] == labels[[2, 3, 4, 5, 7]])), 2]
    got = _run(scores, labels)
    _check(got, want, labels, classes)
    state, confusion, pred, rank, nll = got
    assert state[0] == 5 and state[1] == 3 and state[3] == 2
    assert state[2] == np.sum(pred[[2, 3, 4, 5, 7]] == labels[[2, 3, 4, 5, 7]])
    assert rank[[0, 1, 6]].tolist() == [-1, -1, -1] and nll[[0, 1, 6]].tolist() == [0, 0, 0]
    assert np.array_equal(pred[[0, 1, 6]], np.argmax(scores[[0, 1, 6]], axis=1))
    assert np.isposinf(nll[3]) and np.isnan(nll[4])
    # confusion holds the counted rows only
    assert confusion.sum() == 5
    assert sorted(zip(*np.nonzero(confusion))) == sorted(set(zip(labels[[2, 3, 4, 5, 7]].tolist(),
                                                                 pred[[2, 3, 4, 5, 7]].tolist())))
    assert state[5:].sum() == 5


@pytest.mark.gpu
def test_meter_accumulates_resets_and_merges():
    import torch
    scores, labels, _ = _case(67, 121)
    scores, labels = scores[:10], labels[:10]
    s = torch.from_numpy(np.array(scores)).cuda()
    want = ref.accumulate(scores, labels, 121)

    def same(rep, want, nll):
        assert np.array_equal(rep.state[:4], want[0][:4]) and np.array_equal(rep.state[5:], want[0][5:])
        assert int(rep.state[4]) == ref.q32_sum(nll)
        assert np.array_equal(rep.confusion, want[1])

    one = ClassificationMeter(121, confusion=True)
    pred, rank, nll = one.update(s, torch.from_numpy(np.array(labels)).cuda(), want_rows=True)
    assert pred.is_cuda and pred.dtype == torch.int32 and rank.dtype == torch.int32 and nll.dtype == torch.float32
    assert np.array_equal(pred.cpu().numpy(), want[2]) and np.array_equal(rank.cpu().numpy(), want[3])
    nll = nll.cpu().numpy()
    same(one.result(), want, nll)

    three = ClassificationMeter(121, confusion=True)
    assert three.update(s[:4], labels[:4].tolist()) is None                      # a list, as the loader gives it
    assert three.update(s[4:8], np.array(labels[4:8], dtype=np.int64)) is None   # a numpy array
    assert three.update(s[8:], torch.from_numpy(np.array(labels[8:])).long().cuda()) is None   # device int64
    rep = three.result(top=(1, 5))
    same(rep, want, nll)
    assert np.array_equal(rep.state, one.result().state)
    assert rep.loss == ref.q32_sum(nll) * 2.0 ** -32 / 10
    assert rep.accuracy == float(np.sum(want[2] == labels)) / 10 and rep.top_k(5) == float(np.sum(want[3] < 5)) / 10

    three.reset()
    rep = three.result()
    assert not rep.state.any() and not rep.confusion.any()

    a, b = ClassificationMeter(121, confusion=True), ClassificationMeter(121, confusion=True)
    a.update(s[:6], labels[:6].tolist())
    b.update(s[6:], labels[6:].tolist())
    a.merge(b)
    a.merge(ClassificationMeter(121, confusion=True))    # an empty meter adds nothing
    assert np.array_equal(a.result().state, one.result().state)
    assert np.array_equal(a.result().confusion, want[1])
    fresh = ClassificationMeter(121, confusion=True)
    fresh.merge(b)
    assert np.array_equal(fresh.result().state, b.result().state)

    plain = ClassificationMeter(121)
    plain.update(s, labels.tolist())
    assert plain.result().confusion is None and np.array_equal(plain.result().state, one.result().state)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits():
    import torch
    scores, labels, _ = _case(260, 120)
    s = torch.from_numpy(np.array(scores)).cuda()
    y = torch.from_numpy(np.array(labels)).cuda()
    meters = [ClassificationMeter(120, confusion=True) for _ in range(2)]
    for m in meters:
        m.update(s, y)
    assert torch.equal(meters[0]._state, meters[1]._state)
    assert torch.equal(meters[0]._confusion, meters[1]._confusion)
    assert int(meters[0]._state[0]) == 260


@pytest.mark.gpu
def test_loss_agrees_with_the_training_loss():
    import torch
    from dorknet_amd.layers.losses import SoftmaxWithCrossEntropy
    rng = np.random.RandomState(6)
    logits = rng.randn(6, 120).astype(np.float32)
    y = rng.randint(0, 120, 6)
    onehot = np.eye(120, dtype=np.float32)[y]
    loss, P = SoftmaxWithCrossEntropy("s").forward(torch.from_numpy(logits).cuda(), torch.from_numpy(onehot).cuda())
    meter = ClassificationMeter(120)
    meter.update(P, y)
    rep = meter.result()
    loss = float(loss)
    print("meter loss {!r}, layer loss {!r}, difference {:.3g}, bound {:.3g}".format(
        rep.loss, loss, abs(rep.loss - loss), 2.0 ** -24 * abs(loss) + 2.0 ** -33))
    assert rep.n == 6 and rep.nonfinite == 0
    assert abs(rep.loss - loss) <= 2.0 ** -24 * abs(loss) + 2.0 ** -33


@pytest.mark.gpu
def test_topk_with_scores():
    import torch
    from dorknet_amd._hip import lib, stream_handle
    scores, _, _ = _case(67, 121)
    s = torch.from_numpy(np.array(scores)).cuda()
    idx, val = top_classes_with_scores(s, 5)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and tuple(idx.shape) == tuple(val.shape) == (67, 5)
    assert torch.equal(idx, top_classes(s, 5))
    assert torch.equal(val, s.gather(1, idx.long()))
    tied = torch.from_numpy(np.random.RandomState(2).randint(0, 3, size=(4, 1000)).astype(np.float32)).cuda()
    idx, val = top_classes_with_scores(tied, 16)
    assert np.array_equal(idx.cpu().numpy(), cam_ref.topk_rows(tied.cpu().numpy(), 16))
    assert torch.equal(val, tied.gather(1, idx.long()))
    # the older entry is unchanged: the same indices into a pre-filled buffer
    out = torch.full((4, 16), -7, dtype=torch.int32, device="cuda")
    lib.dk_topk_rows_f32(tied.data_ptr(), 4, 1000, 16, out.data_ptr(), stream_handle())
    assert torch.equal(out, idx)


def _network(X, onehot, seed=0):
    """A seeded ResNet18 after one training forward pass (the running statistics that test_mode reads
    exist from the first batch on)."""
    from examples.resnet18_depsep import ResNet18
    np.random.seed(seed)
    net = ResNet18("eval")
    net.to_gpu()
    net.forward(X, onehot)
    return net


def _train_losses(net, X, onehot):
    """Two training steps' losses (the second sees the first one's update)."""
    import torch
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    sgd = SGDMomentum(net, 0.01, 0.9)
    out = []
    for _ in range(2):
        loss, _ = net.forward(X, onehot)
        net.backward()
        sgd.update_weights()
        out.append(float(loss))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_network_evaluate_and_predict(bf16):
    import torch
    from examples.resnet18_depsep import synthetic_batch
    from tests._convert import all_layers
    X, y, onehot = synthetic_batch(10, size=65)
    X, onehot = torch.as_tensor(X, device="cuda"), torch.as_tensor(onehot, device="cuda")
    if bf16:
        X = X.to(torch.bfloat16)
    net = _network(X, onehot)
    cuts = [(0, 4), (4, 8), (8, 10)]
    scores = np.concatenate([net.forward(X[a:b], None, test_mode=True)[1].cpu().numpy() for a, b in cuts])
    # labels: the network's own answer on every other row, so that correct rows exist; the rest as drawn
    y = np.array(y)
    y[::2] = np.argmax(scores, axis=1)[::2]
    loader = [(X[a:b], y[a:b].tolist(), None) for a, b in cuts]
    loader[1] = (loader[1][0].cpu(), loader[1][1], None)          # one batch from the host
    layers = all_layers(net.layers)
    before = [(l, k, v.clone()) for l in layers for k, v in (l.learned_params or {}).items()]
    stats = [(l, k, v.clone()) for l in layers for k, v in (getattr(l, "non_learned_params", None) or {}).items()
             if isinstance(v, torch.Tensor)]
    assert stats

    rep = net.evaluate(loader, top=(1, 5), confusion=True)
    assert rep.accuracy == net.test(loader, 4, 10)
    assert rep.n == 10 and rep.ignored == 0

    wstate, wconf, wpred, wrank, wnll = ref.accumulate(scores, y, 120)
    assert wstate[2] >= 5
    assert rep.correct == wstate[2] and np.array_equal(rep.rank_hist, wstate[5:]) and np.array_equal(rep.confusion, wconf)
    assert rep.nonfinite == wstate[3]
    fin = np.isfinite(wnll)
    assert abs(rep.loss - wnll[fin].mean()) <= 1e-5 * max(1.0, np.abs(wnll[fin]).max())
    assert rep.top_k(5) == np.sum(wrank < 5) / 10
    assert net.evaluate(loader, num_batches=2).n == 8

    idx, val = net.predict(X[:4], top=5)
    s4 = net.forward(X[:4], None, test_mode=True)[1]
    assert idx.is_cuda and val.is_cuda and tuple(idx.shape) == (4, 5)
    assert torch.equal(idx, top_classes(s4, 5)) and torch.equal(val, s4.gather(1, idx.long()))
    with pytest.raises(ValueError):
        net.predict(X[:4], top=17)

    # the calls change nothing: parameters and running statistics, and the training steps that follow
    # against those of an identical, equally seeded network that never made them
    for l, k, v in before:
        assert torch.equal(l.learned_params[k], v), (l.layer_name, k)
    for l, k, v in stats:
        assert torch.equal(l.non_learned_params[k], v), (l.layer_name, k)
    assert _train_losses(net, X, onehot) == _train_losses(_network(X, onehot), X, onehot)
