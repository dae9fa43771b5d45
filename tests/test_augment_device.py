"""Image augmentation on the GPU: DeviceImageAugmenter and the two entry
points dk_augment_u8 / dk_augment_u8_to_nchw_f32 against tests/_augment_ref.py -- the reference's
four steps applied one after the other in numpy -- bit for bit (np.array_equal): each step alone
and all together, with and without a crop window, to uint8 NHWC and to fp32 NCHW; every colour of
a 64^3 lattice through the HSV step; the CPU known answers again on the GPU; the preprocessing
pipeline with apply_augmenter on and off; and the argument checks, which need no GPU."""
import numpy as np
import pytest

from oracle import pipeline as op
from tests import _augment_ref as ref

HSV = ((0.9, 1.1), (0.5, 2), (0.5, 2))   # the flagship script's augmenter
SHAPES = [(5, 37, 53), (2, 225, 225)]
STEPS = ["hsv", "rotation", "translation", "flip", "all"]


def _augmenter(step):
    from dorknet_amd.data_loading.device_augmentation import DeviceImageAugmenter
    kw = dict(hsv=dict(hsv_pert_tuples=HSV), rotation=dict(rotation_tuple=(-15, 15)),
              translation=dict(translation_tuple=(4, 6)), flip=dict(horizontal_flip_prob=0.5),
              all=dict(hsv_pert_tuples=HSV, rotation_tuple=(-15, 15), translation_tuple=(4, 6),
                       horizontal_flip_prob=0.5))[step]
    return DeviceImageAugmenter(**kw)


def _case(step, N, H, W):
    """Images and per-image parameters that differ, drawn from a fixed seed; with a flip step one image
    is left unflipped and one flipped, with a rotation step one image rotates by exactly 0."""
    rng = np.random.RandomState(1000 + 7 * STEPS.index(step) + N)
    ims = rng.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
    params = _augmenter(step).draw(N, rng)
    if "flip" in params[0]:
        params[0]["flip"], params[1]["flip"] = False, True
    if "rotation" in params[0]:
        params[1]["rotation"] = 0.0
    return ims, params


def _nchw(u8, shift=128.0):
    return u8.astype(np.float32).transpose(0, 3, 1, 2) - np.float32(shift)


def _run(ims, params, crop=None, rows=None, cols=None, f32=False, table=None):
    """The C entry points on a device batch; crop: int32 (N, 2) offsets of a rows x cols window;
    table: a packed parameter table used instead of `params`."""
    import torch
    from dorknet_amd._hip import lib, stream_handle
    from dorknet_amd.data_loading.device_augmentation import DeviceImageAugmenter
    N, H, W, C = ims.shape
    rows, cols = rows or H, cols or W
    x = torch.as_tensor(ims, device="cuda")
    packed = DeviceImageAugmenter.pack(params, rows, cols) if table is None else table
    tab = torch.from_numpy(packed.view(np.uint8)).cuda()
    cr = None if crop is None else torch.as_tensor(np.ascontiguousarray(crop, dtype=np.int32), device="cuda")
    crp = 0 if cr is None else cr.data_ptr()
    if f32:
        out = torch.full((N, 3, rows, cols), float("nan"), dtype=torch.float32, device="cuda")
        lib.dk_augment_u8_to_nchw_f32(x.data_ptr(), N, H, W, C, crp, rows, cols, tab.data_ptr(), 128.0, out.data_ptr(),
                                      stream_handle())
    else:
        out = torch.full((N, rows, cols, 3), 77, dtype=torch.uint8, device="cuda")
        lib.dk_augment_u8(x.data_ptr(), N, H, W, C, crp, rows, cols, tab.data_ptr(), out.data_ptr(), stream_handle())
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("step", STEPS)
def test_augment_bit_exact(step, shape):
    N, H, W = shape
    ims, params = _case(step, N, H, W)
    want = ref.augment_batch(ims, params)
    got = _augmenter(step).augment_batch(ims, params=params)
    assert got.is_cuda and tuple(got.shape) == ims.shape
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(_run(ims, params, f32=True), _nchw(want))
    # a crop window: offsets that differ, one of them the largest that fits
    rows, cols = H - 6, W - 9
    rng = np.random.RandomState(5)
    crop = np.stack([rng.randint(0, 7, N), rng.randint(0, 10, N)], axis=1).astype(np.int32)
    crop[0] = (6, 9)
    wins = np.stack([ims[i, r:r + rows, c:c + cols] for i, (r, c) in enumerate(crop)])
    want = ref.augment_batch(wins, params)
    assert np.array_equal(_run(ims, params, crop, rows, cols), want)
    assert np.array_equal(_run(ims, params, crop, rows, cols, f32=True), _nchw(want))


@pytest.mark.gpu
def test_augment_batch_draws_from_the_given_stream():
    aug = _augmenter("all")
    ims = np.random.RandomState(2).randint(0, 256, size=(3, 19, 23, 3)).astype(np.uint8)
    got = aug.augment_batch(ims, rng=np.random.RandomState(42)).cpu().numpy()
    want = ref.augment_batch(ims, aug.draw(3, np.random.RandomState(42)))
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def lattice():
    """64 values per channel, 0, 1, 254 and 255 among them: 2^18 colours as one 512 x 512 image."""
    vals = np.array(sorted({0, 1, 254, 255} | set(np.round(np.linspace(5, 250, 60)).astype(int).tolist())))
    assert len(vals) == 64
    return np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), axis=-1).reshape(1, 512, 512, 3).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("factors", [(1, 1, 1), (0.9, 0.5, 2), (1.1, 2, 0.5)])
def test_hsv_every_colour_bit_exact(lattice, factors):
    params = [{"hsv": factors}]
    want = ref.augment_batch(lattice, params)
    assert np.array_equal(_run(lattice, params), want)
    assert np.array_equal(_run(lattice, params, f32=True), _nchw(want))


@pytest.mark.gpu
def test_known_answers_on_the_gpu():
    rng = np.random.RandomState(3)
    im = rng.randint(0, 256, size=(1, 13, 17, 3)).astype(np.uint8)
    # all off: a byte copy
    assert np.array_equal(_run(im, [{}]), im)
    assert np.array_equal(_run(im, [{}], f32=True), _nchw(im))
    # rotation by 0 degrees: the identity
    assert np.array_equal(_run(im, [{"rotation": 0.0}]), im)
    # whole-pixel translations: a shifted copy with zero fill; row_trans moves columns
    for row_trans, col_trans in [(0, 0), (3, 0), (0, -2), (-4, 5), (6, 6), (-40, 1), (2, 99)]:
        want = np.zeros_like(im[0])
        H, W = want.shape[:2]
        for y in range(H):
            for x in range(W):
                sy, sx = y - col_trans, x - row_trans
                if 0 <= sy < H and 0 <= sx < W:
                    want[y, x] = im[0, sy, sx]
        assert np.array_equal(_run(im, [{"translation": (row_trans, col_trans)}])[0], want), (row_trans, col_trans)
    # flip
    assert np.array_equal(_run(im, [{"flip": True}])[0], im[0, :, ::-1])
    # rotation by 90 degrees of an 8 x 8 image: rot90 moved down one row, row 0 zero
    sq = rng.randint(0, 256, size=(1, 8, 8, 3)).astype(np.uint8)
    want = np.zeros_like(sq[0])
    want[1:] = np.rot90(sq[0], 1)[:-1]
    assert np.array_equal(_run(sq, [{"rotation": 90.0}])[0], want)


@pytest.mark.gpu
def test_extreme_parameters_stay_in_bounds():
    """A singular or huge matrix and shifts far outside the image read nothing out of bounds and give
    what the restatement gives (coordinates are clamped before they index)."""
    from dorknet_amd.data_loading.device_augmentation import PARAMS_DTYPE
    ims = np.random.RandomState(4).randint(0, 256, size=(4, 11, 9, 3)).astype(np.uint8)
    params = [{"rotation": 33.0, "translation": (2 ** 31 - 1, -(2 ** 31 - 1))}, {"translation": (-9, 0)},
              {"translation": (0, 11), "flip": True}, {"rotation": 180.0}]
    assert np.array_equal(_run(ims, params), ref.augment_batch(ims, params))
    # raw tables: the all-zero (singular) inverse map samples pixel (0, 0) everywhere; huge entries
    # put every tap outside
    tab = np.zeros(4, dtype=PARAMS_DTYPE)
    tab["flags"] = 2
    tab["m"][1] = [1e300, 1e300, 1e300, 1e300, 1e300, 1e300]
    tab["m"][2] = [1.0, 0.0, -1e18, 0.0, 1.0, 1e18]
    tab["m"][3] = [1.0, 0.0, 0.5, 0.0, 1.0, -0.5]
    got = _run(ims, None, table=tab)
    assert np.array_equal(got[0], np.broadcast_to(ims[0, 0, 0], (11, 9, 3)))
    assert not got[1].any() and not got[2].any()
    # a half-pixel map: the mean of four neighbours, (sum + 2) >> 2 up to the 15-bit rounding
    v = ims[3].astype(np.int64)
    pad = np.zeros((13, 11, 3), np.int64)
    pad[1:12, 1:10] = v
    want = (pad[0:11, 1:10] + pad[0:11, 2:11] + pad[1:12, 1:10] + pad[1:12, 2:11]) * 8192
    assert np.array_equal(got[3], (want + 16384) >> 15)


@pytest.mark.gpu
@pytest.mark.parametrize("crop_mode,size,src", [("random", (48, 48), (97, 83)), ("center", (32, 32), (40, 40)),
                                                 (None, (33, 29), (17, 71))])
def test_pipeline_with_augmenter_bit_exact(crop_mode, size, src):
    import torch
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    rng = np.random.RandomState(6)
    N = 4
    ims = rng.randint(0, 256, size=(N, src[0], src[1], 3)).astype(np.uint8)
    aug = _augmenter("all")
    params = aug.draw(N, np.random.RandomState(7))
    params[0]["flip"], params[1]["flip"] = False, True
    pp = DeviceImagePreprocessor(size, crop_mode=crop_mode, image_augmenter=aug, apply_augmenter=True)
    offs = pp.crop_offsets(N, (pp.precrop_size[1], pp.precrop_size[0]), np.random.RandomState(9)) if crop_mode else None
    got = pp.preprocess_batch(torch.as_tensor(ims), offsets=offs, augment_params=params).cpu().numpy()
    want = []
    for i in range(N):
        if crop_mode:
            im = op.resize_bilinear(ims[i], pp.precrop_size[0], pp.precrop_size[1])
            r, c = offs[i]
            im = im[r:r + size[0], c:c + size[1], :]
        else:
            im = op.resize_bilinear(ims[i], size[0], size[1])
        want.append(ref.augment(im, params[i]).astype(np.float32).transpose(2, 0, 1) - np.float32(128))
    want = np.stack(want)
    assert got.shape == want.shape and got.dtype == np.float32 and np.array_equal(got, want)
    # the default: an augmenter that is passed has no effect, bit for bit
    off = DeviceImagePreprocessor(size, crop_mode=crop_mode, image_augmenter=aug)
    plain = np.stack([op.preprocess(ims[i], size, crop_mode, offsets=None if offs is None else tuple(offs[i]))
                      for i in range(N)])
    assert np.array_equal(off.preprocess_batch(torch.as_tensor(ims), offsets=offs).cpu().numpy(), plain)
    none = DeviceImagePreprocessor(size, crop_mode=crop_mode)
    assert np.array_equal(none.preprocess_batch(torch.as_tensor(ims), offsets=offs).cpu().numpy(), plain)


@pytest.mark.gpu
def test_pipeline_draws_interleave_as_in_the_reference():
    """preprocess_image draws the crop's row and column, then calls the augmenter, image by image."""
    import torch
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    ims = np.random.RandomState(8).randint(0, 256, size=(3, 30, 30, 3)).astype(np.uint8)
    aug = _augmenter("all")
    pp = DeviceImagePreprocessor((20, 20), crop_mode="random", precrop_size=(30, 30), image_augmenter=aug,
                                 apply_augmenter=True)
    got = pp.preprocess_batch(torch.as_tensor(ims), rng=np.random.RandomState(10)).cpu().numpy()
    rng = np.random.RandomState(10)
    for i in range(3):
        r, c = rng.randint(0, 10), rng.randint(0, 10)
        p = ref.draw_transcription(rng, HSV, (-15, 15), 0.5, (4, 6))
        want = ref.augment(ims[i, r:r + 20, c:c + 20], p).astype(np.float32).transpose(2, 0, 1) - np.float32(128)
        assert np.array_equal(got[i], want)


def test_bad_arguments_are_refused_without_a_launch():
    """C != 3, missing pointers and a window larger than the image return DK_ERR_ARGS before anything
    touches the device (so this runs without one; the pointers are never dereferenced)."""
    import os
    from dorknet_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip("run __graft_entry__.build() first")
    raw = _hip.lib
    raw._load()
    u8, f32 = raw._lib.dk_augment_u8, raw._lib.dk_augment_u8_to_nchw_f32
    p = 4096  # a non-null address that is never used
    good = dict(src=p, N=2, H=8, W=9, C=3, crop=0, OH=8, OW=9, params=p, dst=p)
    bad = [dict(C=1), dict(C=4), dict(src=0), dict(params=0), dict(dst=0), dict(N=0), dict(OH=9), dict(OW=10),
           dict(OH=0), dict(OW=0), dict(N=-1)]
    for change in bad:
        a = dict(good, **change)
        for fn, extra in ((u8, ()), (f32, (128.0,))):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                fn(a["src"], a["N"], a["H"], a["W"], a["C"], a["crop"], a["OH"], a["OW"], a["params"], *extra, a["dst"], None)


def test_python_argument_checks():
    from dorknet_amd.data_loading.device_augmentation import DeviceImageAugmenter
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    with pytest.raises(ValueError):
        DeviceImagePreprocessor((8, 8), image_augmenter=None, apply_augmenter=True)
    with pytest.raises(ValueError):
        DeviceImagePreprocessor((8, 8), image_augmenter=object(), apply_augmenter=True)
    with pytest.raises(ValueError):
        DeviceImageAugmenter().augment_batch(np.zeros((2, 4, 4, 4), np.uint8))   # C != 3: refused before any device work
    with pytest.raises(ValueError):
        DeviceImageAugmenter.pack([{"hsv": (1.0, float("nan"), 1.0)}], 4, 4)
