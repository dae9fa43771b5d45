"""The device-resident image store and its loader on the GPU: DeviceImageStore,
DeviceImageDataLoader and the entries dk_store_crop_u8, dk_store_batch_nchw_f32, dk_store_batch_nhwc_bf16
and dk_onehot_mixup_f32, bit for bit (np.array_equal) against oracle/pipeline.py (preprocess,
resize_bilinear, mixup) and tests/_augment_ref.py applied image by image: a ragged store whose sizes
take every path of store_pixel in one batch, every crop mode, a non-square size, a real-size case, the
fused mixup of images and labels, bf16 channels-last, the augmented path, a byte offset past 2^31, the
argument checks (no GPU needed) and net.evaluate over the loader."""
import numpy as np
import pytest

from oracle import pipeline as op
from tests import _augment_ref as ref

# source sizes (H, W) for a pre-crop of 60 x 60: copy, 2x2 area, linear, linear, edge clamping on both
# axes, one axis up and one down, and half-area (2x on one axis only), which must go linear
SIZES = [(60, 60), (120, 120), (97, 83), (33, 200), (1, 7), (61, 59), (120, 60)]
LABELS = [3, 0, 2, 2, 1, 0, 3]
HSV = ((0.9, 1.1), (0.5, 2), (0.5, 2))
AUG = dict(hsv_pert_tuples=HSV, rotation_tuple=(-15, 15), horizontal_flip_prob=0.5, translation_tuple=(4, 6))


def _images(sizes, seed, channels=3):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=(h, w, channels)).astype(np.uint8) for h, w in sizes]


@pytest.fixture(scope="module")
def ragged():
    from dorknet_amd.data_loading.device_store import DeviceImageStore
    ims = _images(SIZES, 11)
    return DeviceImageStore.from_arrays(ims, LABELS), ims


def _loaders(store, batch, pp, seed, **kw):
    """Two equally seeded loaders: one plans on the host, the other produces the same batch."""
    from dorknet_amd.data_loading.device_loader import DeviceImageDataLoader
    return [DeviceImageDataLoader(store, batch, pp, class_balance=False, rng=np.random.RandomState(seed), **kw)
            for _ in range(2)]


def _want_half(ims, half, pp, augment=False):
    """The oracle's preprocessing of one planned batch, image by image."""
    out = []
    for (i, r, c), k in zip(half.table.tolist(), range(len(half.table))):
        if augment:
            if pp.crop_mode:
                im = op.resize_bilinear(ims[i], pp.precrop_size[0], pp.precrop_size[1])
                im = im[r:r + pp.image_size[0], c:c + pp.image_size[1], :]
            else:
                im = op.resize_bilinear(ims[i], pp.image_size[0], pp.image_size[1])
            out.append(ref.augment(im, half.augment[k]).astype(np.float32).transpose(2, 0, 1) - np.float32(128))
        else:
            out.append(op.preprocess(ims[i], pp.image_size, pp.crop_mode, pp.precrop_size, offsets=(r, c)))
    return np.stack(out)


def _onehot(labels, classes):
    e = np.zeros((len(labels), classes), dtype=np.float32)
    for n, l in enumerate(labels):
        if 0 <= l < classes:
            e[n, l] = 1
    return e


@pytest.mark.gpu
def test_store_round_trip(ragged):
    import torch
    store, ims = ragged
    assert len(store) == 7 and store.classes == 4 and store.nbytes == sum(im.size for im in ims)
    assert store.data.is_cuda and store.table.is_cuda and store.labels_device.is_cuda
    assert store.labels_device.dtype == torch.int32 and store.labels_device.cpu().tolist() == LABELS
    assert store.shapes.tolist() == [list(s) for s in SIZES]
    for i, im in enumerate(ims):
        assert np.array_equal(store.image(i), im)


@pytest.mark.gpu
@pytest.mark.parametrize("crop_mode,size,precrop", [
    ("random", (48, 48), (60, 60)), ("center", (48, 48), (60, 60)), (None, (48, 48), (60, 60)),
    (None, (60, 60), None),             # no crop at the size at which the copy and area paths run
    ("random", (40, 32), (45, 52)),     # non-square: 40 rows x 32 columns of a resize to 52 rows x 45 columns
    (None, (40, 32), None)], ids=["random", "center", "none", "none60", "random40x32", "none40x32"])
def test_ragged_preprocessing_bit_exact(ragged, crop_mode, size, precrop):
    import torch
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    store, ims = ragged
    pp = DeviceImagePreprocessor(size, crop_mode=crop_mode, precrop_size=precrop)
    planner, loader = _loaders(store, 7, pp, 21)
    plan = planner.plan_batch()
    assert plan.a.indices.tolist() == list(range(7)) and plan.b is None
    (X, y, y1h), = list(loader.pull_batch(1))
    want = _want_half(ims, plan.a, pp)
    assert X.is_cuda and X.dtype == torch.float32 and X.is_contiguous() and tuple(X.shape) == want.shape
    assert np.array_equal(X.cpu().numpy(), want)
    assert y.is_cuda and y.dtype == torch.int32 and y.cpu().tolist() == LABELS
    assert y1h.dtype == torch.float32 and np.array_equal(y1h.cpu().numpy(), np.eye(4, dtype=np.float32)[LABELS])
    if crop_mode == "random":
        assert len({tuple(t) for t in plan.a.table[:, 1:].tolist()}) > 1   # the offsets differ per image


@pytest.mark.gpu
def test_real_size_images_bit_exact():
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    from dorknet_amd.data_loading.device_store import DeviceImageStore
    ims = _images([(375, 500), (333, 500), (500, 375), (360, 480)], 12)
    store = DeviceImageStore.from_arrays(ims, [0, 1, 0, 1])
    pp = DeviceImagePreprocessor((225, 225), crop_mode="random")   # pre-crop 281 x 281
    planner, loader = _loaders(store, 4, pp, 22)
    plan = planner.plan_batch()
    (X, _, _), = list(loader.pull_batch(1))
    assert np.array_equal(X.cpu().numpy(), _want_half(ims, plan.a, pp))


def _crop_u8(ims, batch, TH, TW, OH, OW):
    """dk_store_crop_u8 on a store of `ims`."""
    import torch
    from dorknet_amd._hip import lib, stream_handle
    from dorknet_amd.data_loading.device_store import DeviceImageStore
    store = DeviceImageStore.from_arrays(ims, [0] * len(ims))
    C = store.channels
    tab = torch.as_tensor(np.asarray(batch, dtype=np.int32), device="cuda")
    out = torch.full((len(batch), OH, OW, C), 77, dtype=torch.uint8, device="cuda")
    lib.dk_store_crop_u8(store.data.data_ptr(), store.table.data_ptr(), len(store), C, tab.data_ptr(), len(batch),
                         TH, TW, OH, OW, out.data_ptr(), stream_handle())
    return out.cpu().numpy()


def _crop_want(ims, batch, TH, TW, OH, OW):
    return np.stack([op.resize_bilinear(ims[i], TW, TH)[r:r + OH, c:c + OW, :] for i, r, c in batch])


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_store_crop_u8_is_resize_then_slice(channels):
    ims = _images(SIZES, 13 + channels, channels)
    # every image, some twice, offsets at both ends of their range (0..12) and in between
    batch = [(0, 0, 0), (1, 12, 12), (2, 5, 7), (3, 12, 0), (4, 0, 12), (5, 3, 9), (6, 6, 6), (1, 0, 11), (2, 12, 1)]
    got, want = _crop_u8(ims, batch, 60, 60, 48, 48), _crop_want(ims, batch, 60, 60, 48, 48)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.gpu
def test_a_bad_batch_table_is_clamped():
    """An image index or an offset out of range reads the nearest valid one, never out of bounds."""
    ims = _images(SIZES, 14)
    got = _crop_u8(ims, [(-5, -3, 99), (1000, 99, -1)], 60, 60, 48, 48)
    assert np.array_equal(got, _crop_want(ims, [(0, 0, 12), (6, 12, 0)], 60, 60, 48, 48))


@pytest.mark.gpu
@pytest.mark.parametrize("out", ["fp32", "bf16"])
def test_mixup_fused_bit_exact(ragged, out):
    import torch
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    store, ims = ragged
    pp = DeviceImagePreprocessor((48, 48), crop_mode="random", precrop_size=(60, 60))
    dtype = torch.bfloat16 if out == "bf16" else torch.float32
    planner, loader = _loaders(store, 4, pp, 23, mixup_range_tuple=(0.1, 0.4), out_dtype=dtype)
    plan = planner.plan_batch()
    la, lb = plan.a.labels.tolist(), plan.b.labels.tolist()
    assert plan.a.indices.tolist() == [0, 1, 2, 3] and plan.b.indices.tolist() == [4, 5, 6, 0]
    assert (la, lb) == ([3, 0, 2, 2], [1, 0, 3, 3])                  # the second pair has la == lb
    prop = float(plan.prop)
    A, B = _want_half(ims, plan.a, pp), _want_half(ims, plan.b, pp)
    want_x = op.mixup(A, B, prop)
    eye = np.eye(4, dtype=np.float32)
    want_y = op.mixup(eye[la], eye[lb], prop)
    got = list(loader.pull_batch(2))     # the two mirrored batches, one after the other
    for k in range(2):
        X, y, y1h = got[k]
        assert want_x[k].dtype == np.float32 and tuple(X.shape) == (4, 3, 48, 48) and X.dtype == dtype
        if out == "bf16":
            assert X.is_contiguous(memory_format=torch.channels_last)
            want = torch.from_numpy(want_x[k]).to(torch.bfloat16)
            assert torch.equal(X.cpu().contiguous().view(torch.int16), want.view(torch.int16))
        else:
            assert X.is_contiguous() and np.array_equal(X.cpu().numpy(), want_x[k])
        assert y.cpu().tolist() == (la, lb)[k] and y.dtype == torch.int32
        assert np.array_equal(y1h.cpu().numpy(), want_y[k])
    assert want_y[0][1, 0] == np.float32(prop) + np.float32(1 - prop)


@pytest.mark.gpu
def test_bf16_without_mixup_bit_exact(ragged):
    import torch
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    store, ims = ragged
    pp = DeviceImagePreprocessor((48, 48), crop_mode="center", precrop_size=(60, 60))
    planner, loader = _loaders(store, 7, pp, 24, out_dtype=torch.bfloat16)
    plan = planner.plan_batch()
    (X, _, _), = list(loader.pull_batch(1))
    want = torch.from_numpy(_want_half(ims, plan.a, pp)).to(torch.bfloat16)
    assert X.dtype == torch.bfloat16 and X.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(X.cpu().contiguous().view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("labels,partner", [([0, 4, 2, 7, -1, 5, 8], [3, 4, 9, 7, 2, -6, -3]), ([1, 6, 0, 5, 9, -2], None)],
                         ids=["mixed", "plain"])
def test_onehot_mixup_entry(labels, partner):
    """Same-class pairs give fl(p + q), a label outside [0, classes) a zero row (in either batch)."""
    import torch
    from dorknet_amd._hip import lib, stream_handle
    classes, N, prop = 6, len(labels), 0.3
    p, q = np.float32(prop), np.float32(1 - prop)
    la = torch.as_tensor(np.asarray(labels, np.int32), device="cuda")
    lb = None if partner is None else torch.as_tensor(np.asarray(partner, np.int32), device="cuda")
    ab = torch.full((N, classes), float("nan"), device="cuda")
    ba = torch.full((N, classes), float("nan"), device="cuda")
    lib.dk_onehot_mixup_f32(la.data_ptr(), 0 if lb is None else lb.data_ptr(), N, classes, float(p), float(q),
                            ab.data_ptr(), 0 if lb is None else ba.data_ptr(), stream_handle())
    if partner is None:
        assert np.array_equal(ab.cpu().numpy(), _onehot(labels, classes))
        assert bool(torch.isnan(ba).all())    # not written
    else:
        want = op.mixup(_onehot(labels, classes), _onehot(partner, classes), prop)
        assert np.array_equal(ab.cpu().numpy(), want[0]) and np.array_equal(ba.cpu().numpy(), want[1])
        assert want[0][1, 4] == p + q and not want[0][6].any() and not want[1][3].any()


@pytest.mark.gpu
@pytest.mark.parametrize("crop_mode,mixup", [("random", (0.1, 0.4)), ("center", None), (None, (0.1, 0.4))])
def test_augmented_batches_bit_exact(ragged, crop_mode, mixup):
    from dorknet_amd.data_loading.device_augmentation import DeviceImageAugmenter
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    store, ims = ragged
    pp = DeviceImagePreprocessor((48, 48), crop_mode=crop_mode, precrop_size=(60, 60),
                                 image_augmenter=DeviceImageAugmenter(**AUG), apply_augmenter=True)
    planner, loader = _loaders(store, 4, pp, 25, mixup_range_tuple=mixup)
    plan = planner.plan_batch()
    A = _want_half(ims, plan.a, pp, augment=True)
    eye = np.eye(4, dtype=np.float32)
    if mixup:
        B = _want_half(ims, plan.b, pp, augment=True)
        want_x = op.mixup(A, B, float(plan.prop))
        want_y = op.mixup(eye[plan.a.labels], eye[plan.b.labels], float(plan.prop))
    else:
        want_x, want_y = [A], [eye[plan.a.labels]]
    got = list(loader.pull_batch(len(want_x)))
    for k in range(len(want_x)):
        assert np.array_equal(got[k][0].cpu().numpy(), want_x[k])
        assert np.array_equal(got[k][2].cpu().numpy(), want_y[k])
    # the augmenter did something: the plain preprocessing of the same plan differs
    assert not np.array_equal(A, _want_half(ims, plan.a, pp))


@pytest.mark.gpu
def test_byte_offsets_are_64_bit():
    """One 20 x 30 image at byte offset 2^31 + 4096 of an uninitialised 2^31 + 65536 byte buffer."""
    import torch
    from dorknet_amd._hip import lib, stream_handle
    from dorknet_amd.data_loading.device_store import RECORD_DTYPE, table_to_device
    off = 2 ** 31 + 4096
    im = _images([(20, 30)], 15)[0]
    buf = torch.empty(2 ** 31 + 65536, dtype=torch.uint8, device="cuda")
    buf[off:off + im.size].copy_(torch.from_numpy(im.reshape(-1)))
    rec = np.zeros(1, dtype=RECORD_DTYPE)
    rec["offset"], rec["h"], rec["w"] = off, 20, 30
    table = table_to_device(rec)
    batch = torch.as_tensor(np.asarray([[0, 3, 5], [0, 0, 0]], np.int32), device="cuda")
    TH, TW, OH, OW = 25, 35, 16, 24
    want_u8 = np.stack([op.resize_bilinear(im, TW, TH)[r:r + OH, c:c + OW] for r, c in ((3, 5), (0, 0))])
    u8 = torch.full((2, OH, OW, 3), 77, dtype=torch.uint8, device="cuda")
    f32 = torch.full((2, 3, OH, OW), float("nan"), device="cuda")
    lib.dk_store_crop_u8(buf.data_ptr(), table.data_ptr(), 1, 3, batch.data_ptr(), 2, TH, TW, OH, OW, u8.data_ptr(),
                         stream_handle())
    lib.dk_store_batch_nchw_f32(buf.data_ptr(), table.data_ptr(), 1, 3, batch.data_ptr(), 0, 2, TH, TW, OH, OW, 128.0,
                                0.0, 0.0, f32.data_ptr(), 0, stream_handle())
    assert np.array_equal(u8.cpu().numpy(), want_u8)
    assert np.array_equal(f32.cpu().numpy(), want_u8.astype(np.float32).transpose(0, 3, 1, 2) - np.float32(128))
    # copy mode at the same offset
    same = torch.full((1, 20, 30, 3), 77, dtype=torch.uint8, device="cuda")
    lib.dk_store_crop_u8(buf.data_ptr(), table.data_ptr(), 1, 3, batch.data_ptr(), 1, 20, 30, 20, 30, same.data_ptr(),
                         stream_handle())
    assert np.array_equal(same.cpu().numpy()[0], im)


def test_bad_arguments_are_refused_without_a_launch():
    """Null pointers, N < 1, C outside 1..4, an empty store and a window larger than the target return
    DK_ERR_ARGS before anything touches the device (so this runs without one; the pointers are never
    dereferenced)."""
    import os
    from dorknet_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip("run __graft_entry__.build() first")
    raw = _hip.lib
    raw._load()
    L = raw._lib
    p = 4096  # a non-null address that is never used
    good = dict(data=p, images=p, count=5, C=3, batch=p, partner=p, N=2, TH=10, TW=12, OH=8, OW=9, ab=p, ba=p)
    bad = [dict(data=0), dict(images=0), dict(batch=0), dict(ab=0), dict(count=0), dict(N=0), dict(N=-1), dict(C=0),
           dict(C=5), dict(OH=11), dict(OW=13), dict(OH=0), dict(OW=0), dict(TH=7), dict(TW=8)]
    for change in bad:
        a = dict(good, **change)
        head = (a["data"], a["images"], a["count"], a["C"], a["batch"])
        size = (a["N"], a["TH"], a["TW"], a["OH"], a["OW"])
        with pytest.raises(_hip.HipError, match="bad arguments"):
            L.dk_store_crop_u8(*head, *size, a["ab"], None)
        for fn in (L.dk_store_batch_nchw_f32, L.dk_store_batch_nhwc_bf16):
            for partner in (a["partner"], 0):
                with pytest.raises(_hip.HipError, match="bad arguments"):
                    fn(*head, partner, *size, 128.0, 0.3, 0.7, a["ab"], a["ba"], None)
    for fn in (L.dk_store_batch_nchw_f32, L.dk_store_batch_nhwc_bf16):   # a partner needs the second output
        with pytest.raises(_hip.HipError, match="bad arguments"):
            fn(p, p, 5, 3, p, p, 2, 10, 12, 8, 9, 128.0, 0.3, 0.7, p, 0, None)
    for args in ((0, p, 2, 4, p, p), (p, p, 0, 4, p, p), (p, p, -1, 4, p, p), (p, p, 2, 0, p, p), (p, p, 2, 4, 0, p),
                 (p, p, 2, 4, p, 0)):
        labels, partner, N, classes, y_ab, y_ba = args
        with pytest.raises(_hip.HipError, match="bad arguments"):
            L.dk_onehot_mixup_f32(labels, partner, N, classes, 0.3, 0.7, y_ab, y_ba, None)


@pytest.mark.gpu
def test_network_evaluate_over_the_loader():
    """net.evaluate(loader) over an 8-image ragged store gives the report of the same batches built on the
    host with the oracle, and net.test the same accuracy."""
    import torch
    from dorknet_amd.data_loading.device_loader import DeviceImageDataLoader
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    from dorknet_amd.data_loading.device_store import DeviceImageStore
    from examples.resnet18_depsep import ResNet18
    sizes = SIZES + [(70, 90)]
    ims = _images(sizes, 16)
    labels = [5, 17, 5, 99, 0, 42, 119, 17]
    store = DeviceImageStore.from_arrays(ims, labels, class_names=[str(c) for c in range(120)])
    pp = DeviceImagePreprocessor((65, 65), crop_mode="center", precrop_size=(81, 81))
    host = [(np.stack([op.preprocess(ims[i], (65, 65), "center", (81, 81), offsets=(8, 8)) for i in cut]),
             [labels[i] for i in cut], None) for cut in (range(0, 4), range(4, 8))]
    np.random.seed(0)
    net = ResNet18("loader")
    net.to_gpu()
    onehot = torch.as_tensor(np.eye(120, dtype=np.float32)[labels[:4]], device="cuda")
    net.forward(torch.as_tensor(host[0][0], device="cuda"), onehot)   # running statistics for test_mode
    for dtype in (torch.float32, torch.bfloat16):
        def loader():
            return DeviceImageDataLoader(store, 4, pp, class_balance=False, out_dtype=dtype)
        batches = list(loader())
        assert len(batches) == 2 and batches[1][1].cpu().tolist() == labels[4:]
        got = net.evaluate(loader(), top=(1, 5), confusion=True)
        want = net.evaluate([(torch.as_tensor(X).to(dtype), y, None) for X, y, _ in host], top=(1, 5), confusion=True)
        assert got.n == want.n == 8 and got.correct == want.correct and got.loss == want.loss
        assert np.array_equal(got.rank_hist, want.rank_hist) and np.array_equal(got.confusion, want.confusion)
        assert net.test(loader(), 4, 8) == got.accuracy
