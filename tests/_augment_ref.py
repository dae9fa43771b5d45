"""TEST INFRASTRUCTURE ONLY -- the checker for the device-side image augmentation.  Imported by
tests/ only; the product path (dorknet_amd/data_loading) never calls it.

numpy restatement of the reference's ImageAugmenter (data_loading/image_augmentation.py:16-72):
HSV perturbation, rotation, translation and horizontal flip applied *one after the other*, one
image at a time, each step producing a whole uint8 image -- the order of the reference, and
independent of the index algebra of the one-pass kernel it checks.  Images are BGR, C = 3.

The cv2 calls are restated from OpenCV 4.3 (the reference's pin, opencv-python==4.3.0.36); cv2 is
not installed, so agreement with cv2 itself is unpinned, and this file is the
specification the kernel is pinned to bit for bit:

- cv2.cvtColor BGR2HSV for uint8 (hue range 180): integer work with the two 12-bit division
  tables; COLOR_HSV2BGR for uint8: fp32, one rounding per operation, cvRound (half to even).
- cv2.warpAffine for uint8, INTER_LINEAR, constant border 0, dsize = the input's size: the
  matrix inverted in double as cv2 inverts it, 10-bit fixed-point coordinates quantised to 1/32
  pixel, 15-bit tap weights, (sum + 2^14) >> 15.
- cv2.getRotationMatrix2D((W / 2, H / 2), deg, 1): the centre rounded to fp32, the matrix in
  double.

Per-image parameters are a dict with the keys "hsv" (three factors), "rotation" (degrees),
"translation" ((row_trans, col_trans)) and "flip" (bool); a key that is missing or None skips
its step.  As in the reference, row_trans shifts *columns* and col_trans shifts rows
(translate_image puts row_trans in the x column of the matrix).
"""
from __future__ import annotations

import math

import numpy as np

_F = np.float32
_COORD_MAX = float(1 << 40)  # fixed-point coordinates are clamped here: far outside any image

_i = np.arange(1, 256, dtype=np.float64)
SDIV = np.zeros(256, np.int64)
HDIV = np.zeros(256, np.int64)
SDIV[1:] = np.rint((255 << 12) / (1.0 * _i)).astype(np.int64)   # cvRound: half to even
HDIV[1:] = np.rint((180 << 12) / (6.0 * _i)).astype(np.int64)

# (b, g, r) = tab[...] per hue sector
_SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]], np.int64)


def bgr_to_hsv(im):
    """cv2.cvtColor(im, COLOR_BGR2HSV) for uint8: (h in 0..179, s, v)."""
    v3 = im.astype(np.int64)
    b, g, r = v3[..., 0], v3[..., 1], v3[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    d = v - vmin
    s = (d * SDIV[v] + 2048) >> 12
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h0 * HDIV[d] + 2048) >> 12   # arithmetic shift
    h = h + 180 * (h < 0)
    out = np.stack([h, s, v], axis=-1)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def hsv_to_bgr(hsv):
    """cv2.cvtColor(hsv, COLOR_HSV2BGR) for uint8, fp32 arithmetic."""
    hf = hsv[..., 0].astype(_F) * (_F(6) / _F(180))
    sf = hsv[..., 1].astype(_F) * (_F(1) / _F(255))
    vf = hsv[..., 2].astype(_F) * (_F(1) / _F(255))
    sector = np.floor(hf)
    f = hf - sector
    k = sector.astype(np.int64)
    bad = (k < 0) | (k > 5)
    k[bad] = 0
    f[bad] = 0
    one = _F(1)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))], axis=-1)
    assert tab.dtype == np.float32
    bgr = np.take_along_axis(tab, _SECTOR[k], axis=-1)
    bgr = np.where((hsv[..., 1] == 0)[..., None], vf[..., None], bgr)
    return np.clip(np.rint(bgr * _F(255)), 0, 255).astype(np.uint8)


def perturb_hsv(hsv, factors):
    """hsv_perturbation's fp32 middle: scale, clip to [0, 255], the hue to [0, 179], truncate."""
    x = hsv.astype(np.float32)
    for c in range(3):
        x[..., c] *= _F(factors[c])   # a Python float times a float32 array stays float32
    np.clip(x, 0, 255, out=x)
    np.clip(x[..., 0], 0, 179, out=x[..., 0])
    return x.astype(np.uint8)


def hsv_perturbation(im, factors):
    return hsv_to_bgr(perturb_hsv(bgr_to_hsv(im), factors))


def invert_affine(M):
    """cv2.warpAffine's inversion of the forward 2x3 matrix (double)."""
    m = [float(v) for v in np.asarray(M, np.float64).ravel()]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def _round_fix(v):
    """cvRound to a 64-bit integer, clamped far outside any image (NaN counts as the low end)."""
    return np.fmin(np.fmax(np.rint(v), -_COORD_MAX), _COORD_MAX).astype(np.int64)


def warp_affine(im, M):
    """cv2.warpAffine(im, M, (W, H)) for uint8: INTER_LINEAR, BORDER_CONSTANT 0."""
    H, W = im.shape[:2]
    m = invert_affine(M)
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    X0 = _round_fix((m[1] * ys + m[2]) * 1024) + 16
    Y0 = _round_fix((m[4] * ys + m[5]) * 1024) + 16
    X = (X0[:, None] + _round_fix(m[0] * xs * 1024)[None, :]) >> 5
    Y = (Y0[:, None] + _round_fix(m[3] * xs * 1024)[None, :]) >> 5
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    src = im.astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * ok[..., None]

    w = [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]
    t = [tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)]
    acc = sum(wk[..., None] * tk for wk, tk in zip(w, t))
    return ((acc + 16384) >> 15).astype(np.uint8)


def rotation_matrix(W, H, deg):
    """cv2.getRotationMatrix2D((W / 2, H / 2), deg, 1)."""
    cx, cy = float(_F(W / 2)), float(_F(H / 2))
    a = deg * math.pi / 180
    al, be = math.cos(a), math.sin(a)
    return [[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]]


def rotate_image(im, deg):
    return warp_affine(im, rotation_matrix(im.shape[1], im.shape[0], deg))


def translate_image(im, row_trans, col_trans):
    return warp_affine(im, np.float32([[1, 0, row_trans], [0, 1, col_trans]]))


def augment(im, params):
    """One uint8 (H, W, 3) image through the four steps, in the reference's order."""
    if params.get("hsv") is not None:
        im = hsv_perturbation(im, params["hsv"])
    if params.get("rotation") is not None:
        im = rotate_image(im, params["rotation"])
    if params.get("translation") is not None:
        im = translate_image(im, *params["translation"])
    if params.get("flip"):
        im = im[:, ::-1, :]
    return np.ascontiguousarray(im)


def augment_batch(images, params):
    return np.stack([augment(im, p) for im, p in zip(images, params)])


def draw_transcription(rng, hsv=None, rotation=None, flip_prob=None, translation=None):
    """The draws of one augment() call, in its order (the literal sequence of :17-37 and :69)."""
    p = {}
    if hsv is not None:
        p["hsv"] = (rng.uniform(*hsv[0]), rng.uniform(*hsv[1]), rng.uniform(*hsv[2]))
    if rotation is not None:
        p["rotation"] = rng.uniform(*rotation)
    if translation is not None:
        # random_integers(low, high) is randint(low, high + 1); both draws use the same bounds
        r = rng.randint(-1 * translation[0], translation[1] + 1)
        c = rng.randint(-1 * translation[0], translation[1] + 1)
        p["translation"] = (r, c)
    if flip_prob is not None:
        p["flip"] = bool(rng.uniform() < flip_prob)
    return p
