"""Class activation maps on the GPU: dk_cam_f32 / dk_cam_bf16 and dk_topk_rows_f32
against restatement (a) of tests/_cam_ref.py, bit for bit (np.array_equal), with outputs pre-filled (NaN
masks, 77 overlays) so an unwritten element shows; the Python entry points; the network method; and the
argument checks, which need no GPU."""
import functools
import os

import numpy as np
import pytest

from tests import _cam_ref as ref

from dorknet_amd import _hip
from dorknet_amd.cam import class_activation_maps, top_classes

CLASSES = 10
# (N, K, C, (h, w), (H, W))
SHAPES = {
    "odd": (2, 3, 96, (3, 5), (37, 53)),           # C no multiple of 64, non-square, non-integer scale, ragged tail
    "reference": (1, 3, 512, (8, 8), (225, 225)),  # the reference's own shape
    "shrink": (2, 2, 64, (8, 8), (5, 7)),          # reduction in size
    "copy": (1, 1, 1, (4, 4), (4, 4)),             # equal sizes
    "lds_limit": (1, 1, 130, (32, 32), (33, 31)),  # h * w = 1024
    "wide": (1, 2, 4100, (2, 2), (5, 6)),          # C past the 4096 weights staged in LDS: the rest is read in place
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of a shape, drawn once from a fixed seed: (feat NHWC fp32, weights, class_idx, images)."""
    N, K, C, (h, w), (H, W) = SHAPES[name]
    rng = np.random.RandomState(7 + sorted(SHAPES).index(name))
    feat = np.maximum(rng.standard_normal((N, h, w, C)), 0).astype(np.float32)
    weights = (rng.standard_normal((C, CLASSES)) / np.sqrt(C)).astype(np.float32)
    idx = np.stack([rng.permutation(CLASSES)[:K] for _ in range(N)]).astype(np.int32)
    images = rng.uniform(-128, 127, size=(N, 3, H, W)).astype(np.float32)
    for a in (feat, weights, idx, images):
        a.setflags(write=False)
    return feat, weights, idx, images


def _bf16(a):
    """fp32 values rounded to bf16 (by torch) and widened back: what a bf16 feature map holds."""
    import torch
    return torch.from_numpy(np.array(a)).to(torch.bfloat16).float().numpy()


@functools.lru_cache(maxsize=None)
def _want(name, bf16=False):
    feat, weights, idx, images = _case(name)
    masks, overlays = ref.cam_f32(_bf16(feat) if bf16 else feat, weights, idx, images)
    masks.setflags(write=False)
    overlays.setflags(write=False)
    return masks, overlays


def _run(feat, weights, idx, images, out_size, shift=128.0, mask=True, overlay=True, bf16=False):
    """The C entry point on device copies; outputs pre-filled with NaN / 77."""
    import torch
    from dorknet_amd._hip import lib, stream_handle
    N, h, w, C = feat.shape
    K = idx.shape[1]
    H, W = out_size
    f = torch.from_numpy(np.array(feat)).cuda()
    if bf16:
        f = f.to(torch.bfloat16)
    wt = torch.from_numpy(np.array(weights)).cuda()
    ix = torch.from_numpy(np.array(idx, dtype=np.int32)).cuda()
    im = None if images is None else torch.from_numpy(np.array(images)).cuda()
    m = torch.full((N, K, H, W), float("nan"), dtype=torch.float32, device="cuda") if mask else None
    o = torch.full((N, K, H, W, 3), 77, dtype=torch.uint8, device="cuda") if overlay else None
    entry = lib.dk_cam_bf16 if bf16 else lib.dk_cam_f32
    entry(f.data_ptr(), N, h, w, C, wt.data_ptr(), wt.shape[1], ix.data_ptr(), K, 0 if im is None else im.data_ptr(),
          H, W, float(shift), 0 if m is None else m.data_ptr(), 0 if o is None else o.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    return (None if m is None else m.cpu().numpy()), (None if o is None else o.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_cam_bit_exact(name):
    feat, weights, idx, images = _case(name)
    want_m, want_o = _want(name)
    got_m, got_o = _run(feat, weights, idx, images, SHAPES[name][4])
    assert np.array_equal(got_m, want_m)
    assert np.array_equal(got_o, want_o)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["odd", "reference"])
def test_cam_bf16_features(name):
    feat, weights, idx, images = _case(name)
    want_m, want_o = _want(name, True)
    got_m, got_o = _run(feat, weights, idx, images, SHAPES[name][4], bf16=True)
    assert np.array_equal(got_m, want_m)
    assert np.array_equal(got_o, want_o)


@pytest.mark.gpu
def test_cam_one_output_at_a_time():
    feat, weights, idx, images = _case("odd")
    want_m, want_o = _want("odd")
    got_m, got_o = _run(feat, weights, idx, None, SHAPES["odd"][4], overlay=False)      # mask only, no image
    assert got_o is None and np.array_equal(got_m, want_m)
    got_m, got_o = _run(feat, weights, idx, images, SHAPES["odd"][4], mask=False)       # overlay only
    assert got_m is None and np.array_equal(got_o, want_o)


@pytest.mark.gpu
def test_cam_class_indices():
    feat, weights, _, images = _case("odd")
    size = SHAPES["odd"][4]
    idx = np.array([[1, 1, 4], [7, 2, 7]], dtype=np.int32)      # differ per image, repeat a class
    want_m, want_o = ref.cam_f32(feat, weights, idx, images)
    got_m, got_o = _run(feat, weights, idx, images, size)
    assert np.array_equal(got_m, want_m) and np.array_equal(got_o, want_o)
    assert np.array_equal(got_m[0, 0], got_m[0, 1]) and not np.array_equal(got_m[0, 0], got_m[1, 0])
    bad = np.array([[-3, CLASSES + 89, 2], [2 ** 31 - 1, -2 ** 31, 5]], dtype=np.int32)   # clamped into range
    clamped = np.array([[0, CLASSES - 1, 2], [CLASSES - 1, 0, 5]], dtype=np.int32)
    want_m, want_o = ref.cam_f32(feat, weights, clamped, images)
    got_m, got_o = _run(feat, weights, bad, images, size)
    assert np.array_equal(got_m, want_m) and np.array_equal(got_o, want_o)


@pytest.mark.gpu
def test_cam_negative_weights_take_the_zero_mask_branch():
    feat, weights, idx, images = _case("odd")
    weights = -np.abs(weights)
    want_m, want_o = ref.cam_f32(feat, weights, idx, images)
    assert not want_m.any()
    got_m, got_o = _run(feat, weights, idx, images, SHAPES["odd"][4])
    assert np.array_equal(got_m, want_m) and np.array_equal(got_o, want_o)
    assert not np.signbit(got_m).any()


@pytest.mark.gpu
def test_cam_shift_zero():
    feat, weights, idx, images = _case("odd")
    images = images + np.float32(128)            # already in [0, 255]
    want_m, want_o = ref.cam_f32(feat, weights, idx, images, shift=0.0)
    assert np.array_equal(want_o, _want("odd")[1])
    got_m, got_o = _run(feat, weights, idx, images, SHAPES["odd"][4], shift=0.0)
    assert np.array_equal(got_m, want_m) and np.array_equal(got_o, want_o)


def _topk(scores, k):
    import torch
    from dorknet_amd._hip import lib, stream_handle
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).cuda()
    out = torch.full((s.shape[0], k), -7, dtype=torch.int32, device="cuda")
    lib.dk_topk_rows_f32(s.data_ptr(), s.shape[0], s.shape[1], k, out.data_ptr(), stream_handle())
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 120, 3), (1, 5, 5), (2, 1000, 16)], ids=lambda s: "x".join(map(str, s)))
def test_topk_rows(shape):
    N, classes, K = shape
    rng = np.random.RandomState(classes)
    scores = (rng.permutation(N * classes).reshape(N, classes) - 17).astype(np.float32)    # distinct
    want = np.stack([np.argsort(r)[::-1][:K] for r in scores])
    assert np.array_equal(_topk(scores, K), want)
    assert np.array_equal(top_classes(__import__("torch").from_numpy(scores), K).cpu().numpy(), want)


@pytest.mark.gpu
def test_topk_rows_ties():
    rng = np.random.RandomState(3)
    scores = rng.standard_normal((3, 300)).astype(np.float32)
    scores[0, [5, 250, 299]] = scores[0].max() + 1          # one row holding a tie, at the top
    scores[0, [7, 260]] = scores[0].min()
    scores[1, :] = 0.25                                      # one constant row
    for k in (4, 16):
        assert np.array_equal(_topk(scores, k), ref.topk_rows(scores, k))
    assert _topk(scores, 4)[0, :3].tolist() == [299, 250, 5]
    assert _topk(scores, 4)[1].tolist() == [299, 298, 297, 296]


@pytest.mark.gpu
def test_class_activation_maps_returns_device_tensors():
    import torch
    feat, weights, idx, images = _case("odd")
    N, K, C, (h, w), (H, W) = SHAPES["odd"]
    want_m, want_o = _want("odd")
    f = torch.from_numpy(feat.copy()).cuda().permute(0, 3, 1, 2)     # logical NCHW, channels_last strides
    args = (torch.from_numpy(weights.copy()).cuda(), torch.from_numpy(idx.copy()).cuda())
    im = torch.from_numpy(images.copy()).cuda()
    masks, overlays = class_activation_maps(f, *args, images=im)
    assert masks.is_cuda and masks.dtype == torch.float32 and tuple(masks.shape) == (N, K, H, W)
    assert overlays.is_cuda and overlays.dtype == torch.uint8 and tuple(overlays.shape) == (N, K, H, W, 3)
    assert np.array_equal(masks.cpu().numpy(), want_m) and np.array_equal(overlays.cpu().numpy(), want_o)
    masks, overlays = class_activation_maps(f.contiguous(), *args, out_size=(H, W))   # NCHW memory: converted
    assert overlays is None and np.array_equal(masks.cpu().numpy(), want_m)
    masks, overlays = class_activation_maps(f, *args, images=im, want_masks=False)
    assert masks is None and np.array_equal(overlays.cpu().numpy(), want_o)
    masks, _ = class_activation_maps(f.to(torch.bfloat16), args[0], args[1].long(), out_size=(H, W))
    assert np.array_equal(masks.cpu().numpy(), _want("odd", True)[0])


def test_argument_errors_need_no_gpu():
    import torch
    f = torch.zeros((2, 8, 3, 5))
    wts = torch.zeros((8, 4))
    idx = torch.zeros((2, 3), dtype=torch.int32)
    im = torch.zeros((2, 3, 9, 9))
    bad = [
        dict(features=f[0], dense_weights=wts, class_idx=idx, out_size=(9, 9)),                  # wrong rank
        dict(features=f, dense_weights=wts[:, 0], class_idx=idx, out_size=(9, 9)),
        dict(features=f, dense_weights=wts, class_idx=idx[0], out_size=(9, 9)),
        dict(features=torch.zeros((2, 8, 33, 32)), dense_weights=wts, class_idx=idx, out_size=(9, 9)),   # h w > 1024
        dict(features=f, dense_weights=wts, class_idx=idx),                                      # no size, no images
        dict(features=f, dense_weights=wts, class_idx=idx, out_size=(9, 9), want_masks=False),   # neither output
        dict(features=f, dense_weights=wts, class_idx=idx, images=im[:, :2]),                    # not 3 channels
        dict(features=f, dense_weights=wts, class_idx=idx, images=im.double()),
        dict(features=f, dense_weights=wts, class_idx=idx, images=im, out_size=(8, 9)),
        dict(features=f.to(torch.float16), dense_weights=wts, class_idx=idx, out_size=(9, 9)),
        dict(features=f, dense_weights=torch.zeros((7, 4)), class_idx=idx, out_size=(9, 9)),
        dict(features=f, dense_weights=wts, class_idx=idx.float(), out_size=(9, 9)),
        dict(features=f, dense_weights=wts, class_idx=idx, out_size=(0, 9)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            class_activation_maps(**kw)
    for scores, k in ((torch.zeros(5), 3), (torch.zeros((2, 5)), 0), (torch.zeros((2, 5)), 6), (torch.zeros((2, 40)), 17)):
        with pytest.raises(ValueError):
            top_classes(scores, k)


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")
def test_entry_points_refuse_bad_arguments_without_a_launch():
    lib = _hip.lib
    p = 256   # stands for a device pointer: nothing is launched, so nothing reads it

    def cam(entry=None, N=1, h=3, w=5, C=8, classes=4, K=2, image=p, H=9, W=9, mask=p, overlay=p):
        (entry or lib.dk_cam_f32)(p, N, h, w, C, p, classes, p, K, image, H, W, 128.0, mask, overlay, None)

    for kw in (dict(h=33, w=32), dict(K=0), dict(N=0), dict(H=0), dict(W=0), dict(h=0), dict(w=0), dict(classes=0),
               dict(mask=0, overlay=0), dict(image=0), dict(C=0), dict(H=65536, W=32768)):
        for entry in (lib.dk_cam_f32, lib.dk_cam_bf16):
            with pytest.raises(_hip.HipError, match="10001"):
                cam(entry, **kw)
    for N, classes, K in ((0, 5, 1), (1, 0, 1), (1, 5, 0), (1, 5, 6), (1, 40, 17)):
        with pytest.raises(_hip.HipError, match="10001"):
            lib.dk_topk_rows_f32(p, N, classes, K, p, None)


def _network(X, onehot, seed=0):
    """A seeded ResNet18 after one training forward pass (the running statistics that test_mode reads
    exist from the first batch on)."""
    from examples.resnet18_depsep import ResNet18
    np.random.seed(seed)
    net = ResNet18("cam")
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
def test_network_class_activation_maps(bf16):
    import torch
    from examples.resnet18_depsep import synthetic_batch
    from tests._convert import all_layers
    X, _, onehot = synthetic_batch(2, size=65)
    X, onehot = torch.as_tensor(X, device="cuda"), torch.as_tensor(onehot, device="cuda")
    if bf16:
        X = X.to(torch.bfloat16)
    net = _network(X, onehot)
    before = [(l.layer_name, k, v.clone()) for l in all_layers(net.layers) for k, v in (l.learned_params or {}).items()]
    cls, masks, overlays = net.class_activation_maps(X)
    assert cls.dtype == torch.int32 and tuple(cls.shape) == (2, 3)
    assert tuple(masks.shape) == (2, 3, 65, 65) and tuple(overlays.shape) == (2, 3, 65, 65, 3)

    # by hand
    _, scores = net.forward(X, None, test_mode=True)
    _, feats = net.forward(X, None, test_mode=True, terminal_layer_name="res8")
    assert feats.dtype == (torch.bfloat16 if bf16 else torch.float32) and feats.shape[1] == 512
    dense = next(l for l in net.layers if l.layer_name == "dense1")
    idx = top_classes(scores, 3)
    m2, o2 = class_activation_maps(feats, dense.learned_params["weights"], idx, images=X.float())
    assert torch.equal(cls, idx) and torch.equal(masks, m2) and torch.equal(overlays, o2)

    # restatement (a) on host copies
    assert np.array_equal(cls.cpu().numpy(), ref.topk_rows(scores.cpu().numpy(), 3))
    want_m, want_o = ref.cam_f32(feats.permute(0, 2, 3, 1).float().cpu().numpy(),
                                 dense.learned_params["weights"].cpu().numpy(), cls.cpu().numpy(),
                                 X.float().cpu().numpy())
    assert np.array_equal(masks.cpu().numpy(), want_m) and np.array_equal(overlays.cpu().numpy(), want_o)

    # the call changes nothing: the parameters, and the training steps that follow against those of an
    # identical, equally seeded network that never made it
    for name, k, v in before:
        layer = next(l for l in all_layers(net.layers) if l.layer_name == name)
        assert torch.equal(layer.learned_params[k], v), (name, k)
    assert _train_losses(net, X, onehot) == _train_losses(_network(X, onehot), X, onehot)

    for kw in (dict(dense_layer="dense9"), dict(dense_layer="res8"), dict(feature_layer="res9")):
        with pytest.raises(ValueError, match=list(kw.values())[0]):
            net.class_activation_maps(X, **kw)
