"""Class activation maps restated in numpy: what dk_cam_f32 / dk_cam_bf16 and
dk_topk_rows_f32 (dorknet_amd/csrc/cam.hip) compute, and what they are measured against.

Two restatements of the reference's returnCAM + show_cam_on_image
(examples/imagenet_dogs_225_resnet_18_depsep_CAM.py:13-49):

(a) ``cam_f32``: the kernel's own arithmetic, fp32 with one rounding per operation and the kernel's
    summation order.  The kernel must match it with np.array_equal.
(b) ``cam_f64``: the reference's code path in fp64 (np.dot for the dot product, the same resize rule
    and colour table).  (a) is held to (b) within the bounds derived below.

Both share the definition (nothing here calls cv2: it is not installed, so agreement with cv2's own
resize and COLORMAP_JET is unpinned):

- dot product at map position p, (a) only: 64 partial sums s_j = 0; s_j = s_j + w[c] * f[p][c] for
  c = j, j + 64, ... ascending (product rounded, then the sum); s_j = s_j + s_{j+d} for
  d = 32, 16, 8, 4, 2, 1; the result is s_0.
- cv2.resize INTER_LINEAR, fp32 (OpenCV 4.3): scale = (double)L / O; f = (float)((o + 0.5) * scale - 0.5);
  s = floor(f); f -= s; s < 0 -> (0, 0); s >= L - 1 -> (L - 1, 0) with the second tap's index clamped;
  the same rule for rows and columns; t = S[sx] * (1 - fx) + S[sx + 1] * fx on both rows, then
  u = t0 * (1 - fy) + t1 * fy.
- v = max(u, 0); mn, mx over the map; m = v - mn; m = m / (mx - mn) if mx - mn > 0.
- i = (uint8)(255 * m); heat = JET[i]; o = heat + (image + shift) per channel (B, G, R);
  M = max o; out = (uint8)(255 * (o / M)), clamped to [0, 255] (a NaN takes 0).
- JET[i] = round_half_even(255 * (b, g, r)) with b = clamp01(min(i + 32, 160 - i) / 64),
  g = clamp01(min(i - 31, 224 - i) / 64), r = b[255 - i].

Bounds of (a) against (b)  (u = 2^-24, gamma_k = k u / (1 - k u); both see the same fp32 inputs)

Mask.  1. Dot product.  A sum of C rounded products, in any order, obeys
          |S_a[p] - S_b[p]| <= e[p] = gamma_C * sum_c |w_c| |f_pc|            (Higham, Accuracy and Stability, (3.5))
       2. Interpolation.  u = sum_i c_i S_i over four taps with c_i >= 0, sum c_i = 1.  In fp32 each tap
          passes at most six roundings (1 - fx, product, sum, 1 - fy, product, sum), and (b)'s own fp64
          roundings are below one more fp32 rounding, so with I[.] the same interpolation applied in fp64
              |u_a - u_b| <= E = I[e] + gamma_7 * I[|S_b| + e].
          max(., 0) is 1-Lipschitz: |v_a - v_b| <= E per pixel, and with Emax = max over pixels of E,
          |mn_a - mn_b| <= Emax and |mx_a - mx_b| <= Emax.
       3. Normalisation.  n = v - mn: |n_a - n_b| <= En = E + Emax + u (n_b + E + Emax).
          R = mx - mn:    |R_a - R_b| <= ER = 2 Emax + u (R_b + 2 Emax).
          m = n / R with m_b <= 1 and m_a <= 1, one more rounding for the quotient:
              |m_a - m_b| <= (En + m_b ER) / (R_b - ER) + u                     (needs R_b > ER)
          -- the error of the map amplified by 1 / (mx - mn).  ``mask_bound`` returns this per element.
Overlay.  With 255 * (mask bound) + 255 u < 1 the table index differs by at most one, so a heat channel
       differs by at most s, the largest step between neighbouring table entries.  image + shift and
       heat + (.) are below 512, two roundings of at most 2^-16 each, so |o_a - o_b| <= d = s + 2^-15,
       and the same for the maximum M.  For q = 255 o / M with o_b <= M_b:
           |q_a - q_b| <= 255 (d / M_a + (o_b / M_b) d / M_a) + 2^-15 <= 510 d / (M_b - d) + 2^-15
       (quotient and product below 256, two roundings), and truncation adds at most one level:
           |out_a - out_b| <= floor(510 d / (M_b - d) + 2^-15) + 1.            ``overlay_levels``
"""
import numpy as np

U32 = 2.0 ** -24


def gamma(k):
    return k * U32 / (1 - k * U32)


def jet_table():
    """COLORMAP_JET as defined above: uint8 (256, 3), BGR."""
    i = np.arange(256, dtype=np.float64)
    b = np.clip(np.minimum(i + 32, 160 - i) / 64, 0, 1)
    g = np.clip(np.minimum(i - 31, 224 - i) / 64, 0, 1)
    r = b[::-1]
    return np.rint(255 * np.stack([b, g, r], axis=1)).astype(np.uint8)   # np.rint rounds half to even


JET = jet_table()
JET_STEP = int(np.abs(np.diff(JET.astype(np.int64), axis=0)).max())   # s of the overlay bound


def axis(O, L):
    """The taps of output coordinates 0 .. O - 1 on a source axis of length L: (s0, s1, f fp32)."""
    scale = np.float64(L) / np.float64(O)
    f = ((np.arange(O, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    f = f - fl
    lo = s < 0
    s[lo], f[lo] = 0, 0
    hi = s >= L - 1
    s[hi], f[hi] = L - 1, 0
    return s, np.minimum(s + 1, L - 1), f.astype(np.float32)


def resize(S, H, W, dtype=np.float32):
    """cv2.resize(S, (W, H)) INTER_LINEAR as defined above, arithmetic in `dtype` (the tap fractions are
    the fp32 ones either way)."""
    S = np.asarray(S, dtype=dtype)
    h, w = S.shape
    x0, x1, fx = axis(W, w)
    y0, y1, fy = axis(H, h)
    fx, fy = fx.astype(dtype), fy.astype(dtype)
    one = dtype(1)
    t = S[:, x0] * (one - fx) + S[:, x1] * fx                       # (h, W)
    return t[y0] * (one - fy)[:, None] + t[y1] * fy[:, None]        # (H, W)


def dot_map_f32(f, wcol):
    """The kernel's dot product: f (P, C) fp32, wcol (C,) fp32 -> (P,) fp32."""
    f = np.asarray(f, dtype=np.float32)
    wcol = np.asarray(wcol, dtype=np.float32)
    P, C = f.shape
    s = np.zeros((P, 64), dtype=np.float32)
    for c0 in range(0, C, 64):
        k = min(64, C - c0)
        s[:, :k] = s[:, :k] + wcol[None, c0:c0 + k] * f[:, c0:c0 + k]
    for d in (32, 16, 8, 4, 2, 1):
        s[:, :d] = s[:, :d] + s[:, d:2 * d]
    return s[:, 0].copy()


def _level(r):
    """(uint8)r truncating, clamped to [0, 255]; a NaN takes 0."""
    with np.errstate(invalid="ignore"):
        return np.where(r >= 0, np.minimum(r, 255), 0).astype(np.int64)


def _normalise(v, dtype):
    mn, mx = v.min(), v.max()
    rng = dtype(mx - mn)
    m = v - mn
    if rng > 0:
        m = m / rng
    return m.astype(dtype)


def _overlay(m, image_hw3, shift, dtype):
    heat = JET[_level(dtype(255) * m)].astype(dtype)
    o = heat + (image_hw3.astype(dtype) + dtype(shift))
    with np.errstate(invalid="ignore", divide="ignore"):
        return _level(dtype(255) * (o / o.max())).astype(np.uint8)


def _clip_idx(class_idx, classes):
    return np.clip(np.asarray(class_idx, dtype=np.int64), 0, classes - 1)


def cam_f32(feat, weights, class_idx, images=None, out_size=None, shift=128.0, want_masks=True):
    """(a): feat (N, h, w, C) fp32 (bf16 features widened first), weights (C, classes) fp32, class_idx
    (N, K), images (N, 3, H, W) fp32 or None -> (masks fp32 (N, K, H, W) | None, overlays uint8
    (N, K, H, W, 3) | None)."""
    feat = np.asarray(feat, dtype=np.float32)
    weights = np.asarray(weights, dtype=np.float32)
    N, h, w, C = feat.shape
    idx = _clip_idx(class_idx, weights.shape[1])
    K = idx.shape[1]
    H, W = out_size if out_size is not None else images.shape[2:]
    masks = np.empty((N, K, H, W), dtype=np.float32)
    overlays = None if images is None else np.empty((N, K, H, W, 3), dtype=np.uint8)
    for n in range(N):
        for k in range(K):
            S = dot_map_f32(feat[n].reshape(h * w, C), weights[:, idx[n, k]]).reshape(h, w)
            u = resize(S, H, W)
            v = np.where(u > 0, u, np.float32(0))
            masks[n, k] = m = _normalise(v, np.float32)
            if images is not None:
                overlays[n, k] = _overlay(m, np.asarray(images[n], np.float32).transpose(1, 2, 0), shift, np.float32)
    return (masks if want_masks else None), overlays


def return_cam_f64(feature_conv, weight_softmax, class_idx, size_upsample):
    """The reference's returnCAM (:13-32) in fp64: feature_conv (1, chans, height, width), weight_softmax
    (classes, chans), size_upsample (W, H) as cv2.resize takes it."""
    bz, chans, height, width = feature_conv.shape
    output_cam = []
    for idx in class_idx:
        cam = weight_softmax[idx, :].dot(feature_conv.reshape((chans, height * width)))
        cam = cam.reshape(height, width)
        cam = resize(cam, size_upsample[1], size_upsample[0], dtype=np.float64)
        cam = np.maximum(cam, 0)
        cam = cam - np.min(cam)
        if np.max(cam) > 0:
            cam_img = cam / np.max(cam)
        else:
            cam_img = cam
        output_cam.append(cam_img)
    return output_cam


def show_cam_on_image_f64(img, mask):
    """The reference's show_cam_on_image (:43-49) in fp64: img (H, W, 3), mask (H, W)."""
    heatmap = JET[np.uint8(255 * mask)].astype(np.float64)
    cam = heatmap + np.float64(img)
    cam = cam / np.max(cam)
    return np.uint8(255 * cam)


def cam_f64(feat, weights, class_idx, images=None, out_size=None, shift=128.0):
    """(b): the reference's two functions in fp64, image by image, on the arguments of cam_f32.  Returns
    (masks fp64 (N, K, H, W), overlays uint8 | None, aux) with aux the per-map quantities the bounds need:
    'S' (N, K, h, w) the fp64 maps, 'A' (N, K, h, w) sum_c |w_c| |f_pc|, 'M' (N, K) the overlay maxima."""
    feat = np.asarray(feat, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.float64)
    N, h, w, C = feat.shape
    idx = _clip_idx(class_idx, weights.shape[1])
    K = idx.shape[1]
    H, W = out_size if out_size is not None else images.shape[2:]
    dense_weights = weights.reshape((-1, weights.shape[1])).transpose(1, 0)   # the reference's :64
    masks = np.empty((N, K, H, W), dtype=np.float64)
    overlays = None if images is None else np.empty((N, K, H, W, 3), dtype=np.uint8)
    aux = {"S": np.empty((N, K, h, w)), "A": np.empty((N, K, h, w)), "M": np.zeros((N, K))}
    for n in range(N):
        fc = feat[n].transpose(2, 0, 1)[None]                               # (1, C, h, w)
        cams = return_cam_f64(fc, dense_weights, idx[n], (W, H))
        for k, cam in enumerate(cams):
            masks[n, k] = cam
            aux["S"][n, k] = dense_weights[idx[n, k]].dot(fc.reshape(C, h * w)).reshape(h, w)
            aux["A"][n, k] = np.abs(dense_weights[idx[n, k]]).dot(np.abs(fc.reshape(C, h * w))).reshape(h, w)
            if images is not None:
                img = np.asarray(images[n], np.float64).transpose(1, 2, 0) + shift   # the reference's :84
                overlays[n, k] = show_cam_on_image_f64(img, cam)
                aux["M"][n, k] = (JET[np.uint8(255 * cam)].astype(np.float64) + img).max()
    return masks, overlays, aux


def mask_bound(S, A, C, H, W, mask_b):
    """The per-element bound on |mask_a - mask_b| of one map (the docstring's steps 1-3): S, A the fp64
    map and its sum of magnitudes (h, w), mask_b the fp64 mask (H, W).  Returns (bound (H, W), R_b, ER);
    the bound holds where R_b > ER."""
    e = gamma(C) * A
    E = resize(e, H, W, dtype=np.float64) + gamma(7) * resize(np.abs(S) + e, H, W, dtype=np.float64)
    Emax = E.max()
    v = np.maximum(resize(S, H, W, dtype=np.float64), 0)
    Rb = v.max() - v.min()
    nb = v - v.min()
    En = E + Emax + U32 * (nb + E + Emax)
    ER = 2 * Emax + U32 * (Rb + 2 * Emax)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = (En + mask_b * ER) / (Rb - ER) + U32
    return bound, Rb, ER


def overlay_levels(M_b, step=None):
    """The bound on |overlay_a - overlay_b| in levels for a map whose fp64 maximum of heat + image is M_b."""
    d = (JET_STEP if step is None else step) + 2.0 ** -15
    return int(np.floor(510 * d / (M_b - d) + 2.0 ** -15)) + 1


def topk_rows(scores, k):
    """np.argsort(row)[::-1][:k] per row (stable, so of equal scores the higher index comes first)."""
    scores = np.asarray(scores)
    return np.stack([np.argsort(r, kind="stable")[::-1][:k] for r in scores]).astype(np.int32)
