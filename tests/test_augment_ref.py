"""Image augmentation, CPU side: tests/_augment_ref.py -- the numpy
restatement of the reference's ImageAugmenter that pins the HIP kernel bit for bit -- is itself
pinned here by known answers, by exactness of bilinear interpolation on a ramp (against the
analytic value and scipy.ndimage.affine_transform), by colorsys for BGR -> HSV, and
DeviceImageAugmenter.draw by a literal transcription of augment's draw sequence.  cv2 is not
installed, so nothing here compares against cv2 (parity with cv2 itself is unpinned)."""
import colorsys
import math

import numpy as np
import pytest

from tests import _augment_ref as ref


def _rand_image(seed, H, W):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


def shifted_copy(im, row_trans, col_trans):
    """The reference's translate_image as an explicit copy: row_trans moves columns (x),
    col_trans moves rows (y), zero fill."""
    H, W = im.shape[:2]
    out = np.zeros_like(im)
    for y in range(H):
        for x in range(W):
            sy, sx = y - col_trans, x - row_trans
            if 0 <= sy < H and 0 <= sx < W:
                out[y, x] = im[sy, sx]
    return out


def test_rotation_by_zero_is_identity():
    for (H, W) in [(8, 8), (37, 53), (41, 57)]:
        im = _rand_image(0, H, W)
        assert np.array_equal(ref.rotate_image(im, 0.0), im)


@pytest.mark.parametrize("row_trans,col_trans", [(0, 0), (3, 0), (0, -2), (-4, 5), (6, 6), (-40, 1), (2, 99)])
def test_integer_translation_is_a_shifted_copy(row_trans, col_trans):
    im = _rand_image(1, 13, 17)
    assert np.array_equal(ref.translate_image(im, row_trans, col_trans), shifted_copy(im, row_trans, col_trans))


def test_translation_quirk_row_trans_moves_columns():
    im = _rand_image(2, 6, 9)
    out = ref.translate_image(im, 2, 0)          # "row" translation of 2 ...
    assert np.array_equal(out[:, 2:], im[:, :-2])  # ... moves the image two columns to the right
    assert not out[:, :2].any()


def test_rotation_by_90_degrees_8x8():
    # centre (4, 4): (x, y) -> source (7 - y + 1, x) = rot90 moved down one row, row 0 from outside
    im = _rand_image(3, 8, 8)
    want = np.zeros_like(im)
    want[1:] = np.rot90(im, 1)[:-1]
    assert np.array_equal(ref.rotate_image(im, 90.0), want)


RAMP_H, RAMP_W = 41, 57
RAMP_COEF = np.array([[20, 2, 1], [30, 1, 2], [10, 3, 0]], np.float64)  # c0 + cx * x + cy * y per channel


def _ramp(xs, ys):
    return np.stack([c0 + cx * xs + cy * ys for c0, cx, cy in RAMP_COEF], axis=-1)


@pytest.mark.parametrize("deg", [-15, -7.3, 0.5, 3, 11.9, 15])
def test_rotation_is_exact_on_a_ramp(deg):
    """Bilinear interpolation reproduces a linear ramp, so the output is the ramp at the exact source
    coordinate: 1/32-pixel coordinate quantisation moves it by at most 1/64 pixel per axis, times a
    gradient sum of at most 3 per channel = 3/64, plus 0.5 of output rounding: |diff| < 1 wherever the
    four taps are inside."""
    H, W = RAMP_H, RAMP_W
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    im = _ramp(xs, ys)
    assert im.max() <= 255
    im = im.astype(np.uint8)
    out = ref.rotate_image(im, deg).astype(np.float64)
    # the exact inverse map of a rotation by deg about (W / 2, H / 2)
    a = math.radians(deg)
    cx, cy = W / 2, H / 2
    sx = math.cos(a) * (xs - cx) - math.sin(a) * (ys - cy) + cx
    sy = math.sin(a) * (xs - cx) + math.cos(a) * (ys - cy) + cy
    # all four taps inside, with the quantised coordinate at most 1/32 away
    inside = (sx >= 0.05) & (sx <= W - 1.05) & (sy >= 0.05) & (sy <= H - 1.05)
    assert inside.sum() > 0.6 * H * W
    worst = np.abs(out - _ramp(sx, sy))[inside].max()
    print("ramp", deg, "max |diff| vs the analytic ramp", worst)
    assert worst < 1
    from scipy import ndimage
    # affine_transform maps output (row, col) to input (row, col): the same inverse map
    mat = np.array([[math.cos(a), math.sin(a)], [-math.sin(a), math.cos(a)]])
    off = np.array([cy, cx]) - mat @ np.array([cy, cx])
    for c in range(3):
        sp = ndimage.affine_transform(im[..., c].astype(np.float64), mat, offset=off, order=1, mode="constant", cval=0.0)
        w = np.abs(out[..., c] - sp)[inside].max()
        print("ramp", deg, "channel", c, "max |diff| vs scipy", w)
        assert w < 1


def test_bgr_to_hsv_against_colorsys():
    vals = sorted({0, 1, 2, 127, 128, 254, 255} | set(range(3, 254, 10)))
    g = np.array(vals, np.uint8)
    bgr = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 1, 3)
    hsv = ref.bgr_to_hsv(bgr).reshape(-1, 3).astype(np.float64)
    worst_h = worst_s = 0.0
    for (b, gg, r), (h, s, v) in zip(bgr.reshape(-1, 3), hsv):
        ch, cs, cv = colorsys.rgb_to_hsv(r / 255.0, gg / 255.0, b / 255.0)
        assert v == max(b, gg, r) == round(cv * 255)
        dh = abs(h - ch * 180.0)
        worst_h = max(worst_h, min(dh, 180.0 - dh))   # hue is circular
        worst_s = max(worst_s, abs(s - cs * 255.0))
    print("BGR -> HSV vs colorsys: hue", worst_h, "saturation", worst_s)
    assert worst_h < 1 and worst_s < 1


def test_hue_maximum_is_179():
    g = np.arange(256, dtype=np.uint8)
    # red is the maximum and blue just above green: the hues just below 360 degrees
    bgr = np.stack(np.meshgrid(g, g, np.array([255, 200, 64, 3], np.uint8), indexing="ij"), axis=-1).reshape(-1, 1, 3)
    hsv = ref.bgr_to_hsv(bgr)
    assert hsv[..., 0].max() == 179
    assert ref.perturb_hsv(hsv, (2.0, 1.0, 1.0))[..., 0].max() == 179   # clipped after the scale


def test_division_tables():
    assert ref.SDIV[0] == 0 and ref.HDIV[0] == 0
    assert ref.SDIV[255] == 4096 and ref.SDIV[1] == 255 << 12
    assert ref.HDIV[1] == 122880 and ref.HDIV[255] == 482
    # integer restatement of cvRound (half to even) of the quotient, as the kernel builds them
    for i in range(1, 256):
        for n, den, tab in (((255 << 12), i, ref.SDIV), ((180 << 12), 6 * i, ref.HDIV)):
            q, rem = divmod(n, den)
            q += 1 if (2 * rem > den or (2 * rem == den and q & 1)) else 0
            assert tab[i] == q


def test_hsv_round_trip_of_greys_and_primaries():
    greys = np.arange(256, dtype=np.uint8)[:, None, None].repeat(3, axis=2)
    assert np.array_equal(ref.hsv_perturbation(greys, (1, 1, 1)), greys)          # s == 0: b = g = r = v
    prim = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]], np.uint8)
    assert np.array_equal(ref.hsv_perturbation(prim, (1, 1, 1)), prim)
    assert np.array_equal(ref.hsv_perturbation(prim, (1, 1, 0.5)), np.where(prim > 0, 127, 0))   # v = 127.5 truncated


def test_sequential_order_and_flip():
    im = _rand_image(4, 9, 11)
    p = {"translation": (2, -1), "flip": True}
    assert np.array_equal(ref.augment(im, p), shifted_copy(im, 2, -1)[:, ::-1])
    assert np.array_equal(ref.augment(im, {}), im)
    assert np.array_equal(ref.augment(im, {"flip": False}), im)


OPTIONS = [
    dict(hsv_pert_tuples=((0.9, 1.1), (0.5, 2), (0.5, 2)), rotation_tuple=(-15, 15), horizontal_flip_prob=0.5,
         translation_tuple=(4, 6)),
    dict(hsv_pert_tuples=((0.9, 1.1), (0.5, 2), (0.5, 2)), rotation_tuple=(-15, 15), horizontal_flip_prob=0.5),
    dict(rotation_tuple=(-3, 8)),
    dict(translation_tuple=(2, 7), horizontal_flip_prob=0.3),
    dict(hsv_pert_tuples=((1, 1), (0.5, 2), (1, 1))),
    dict(),
]


@pytest.mark.parametrize("opts", OPTIONS)
def test_draw_consumes_the_stream_as_the_reference_does(opts):
    from dorknet_amd.data_loading.device_augmentation import DeviceImageAugmenter
    aug = DeviceImageAugmenter(**opts)
    a, b = np.random.RandomState(11), np.random.RandomState(11)
    got = aug.draw(7, a)
    want = [ref.draw_transcription(b, opts.get("hsv_pert_tuples"), opts.get("rotation_tuple"),
                                   opts.get("horizontal_flip_prob"), opts.get("translation_tuple")) for _ in range(7)]
    assert got == want
    assert a.uniform() == b.uniform()   # both streams stand at the same place
    if "translation_tuple" in opts:
        lo, hi = -opts["translation_tuple"][0], opts["translation_tuple"][1]
        assert all(lo <= v <= hi for p in got for v in p["translation"])


def test_draw_defaults_to_the_global_stream():
    from dorknet_amd.data_loading.device_augmentation import DeviceImageAugmenter
    aug = DeviceImageAugmenter(**OPTIONS[0])
    np.random.seed(5)
    got = aug.draw(3)
    assert got == aug.draw(3, np.random.RandomState(5))


def test_pack_matches_the_restated_matrices():
    from dorknet_amd.data_loading.device_augmentation import (FLAG_FLIP, FLAG_HSV, FLAG_ROTATE, PARAMS_DTYPE,
                                                               DeviceImageAugmenter)
    assert PARAMS_DTYPE.itemsize == 72
    ps = [{"hsv": (0.9, 0.5, 2.0), "rotation": 11.9, "translation": (3, -2), "flip": True}, {"rotation": 0.0}, {}]
    tab = DeviceImageAugmenter.pack(ps, 37, 53)
    assert tab["flags"].tolist() == [FLAG_HSV | FLAG_ROTATE | FLAG_FLIP, FLAG_ROTATE, 0]
    assert (tab["tx"][0], tab["ty"][0]) == (3, -2)       # row_trans shifts columns
    assert tab["m"][0].tolist() == ref.invert_affine(ref.rotation_matrix(53, 37, 11.9))
    assert tab["m"][1].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert tab["hsv"][0].tolist() == [float(np.float32(v)) for v in (0.9, 0.5, 2.0)]
    with pytest.raises(ValueError):
        DeviceImageAugmenter.pack([{"translation": (1.5, 0)}], 8, 8)
