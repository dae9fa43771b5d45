"""Device-side image augmentation.

Reference: ``ImageAugmenter`` (data_loading/image_augmentation.py:4-72) perturbs one decoded
uint8 BGR image on the host with OpenCV -- HSV perturbation (:41-50), rotation about the centre
(:61-66), integer translation (:52-59) and a horizontal flip (:68-72), in that order, each a
whole-image pass.  ``DeviceImageAugmenter`` takes the same constructor keywords, draws the same
random numbers in the same order, and runs all four steps for a whole uint8 NHWC batch in one
HIP kernel (dk_augment_u8 / dk_augment_u8_to_nchw_f32 in dorknet_amd/csrc/input_pipeline.hip):
the HSV step is per pixel, an integer translation is an index shift and the flip an index
mirror, so each output pixel is the rotation's (up to) four taps of HSV-perturbed source pixels
at a shifted, mirrored position -- the image is read once and written once.

- ``draw(n, rng=np.random)``: the parameters of n images, one dict each with the keys the
  enabled options produce: "hsv" (three factors), "rotation" (degrees), "translation"
  ((row_trans, col_trans)), "flip" (bool).  Per image: three uniforms, one uniform, two randint,
  one uniform -- the draws of ``augment`` (:17-37, :69), so a seeded loop written against the
  reference sees the same stream.
- ``augment_batch(images, rng=np.random, params=None)``: uint8 (N, H, W, 3) in, the augmented
  uint8 batch on the GPU out.

Quirk kept from the reference: ``translate_image`` puts row_trans into the x column of its
matrix, so row_trans shifts *columns* and col_trans shifts rows, and both are drawn with the
bounds (-translation_tuple[0], translation_tuple[1]).

The cv2 calls are restated from OpenCV 4.3 (tests/_augment_ref.py pins the kernel bit for bit);
cv2 is not installed to compare against, so agreement with cv2 itself is unpinned.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .._hip import lib, stream_handle

# one record per image, the layout of dk_augment_params in include/dorknet_hip.h
PARAMS_DTYPE = np.dtype([("m", "<f8", (6,)), ("hsv", "<f4", (3,)), ("tx", "<i4"), ("ty", "<i4"), ("flags", "<i4")])
FLAG_HSV, FLAG_ROTATE, FLAG_FLIP = 1, 2, 4
_INT_MAX = 2 ** 31 - 1


def invert_affine(M):
    """The inverse map of a forward 2x3 matrix, as cv2.warpAffine forms it in double."""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11 = m[4] * D
    A22 = m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2] = b1
    m[5] = b2
    return m


def rotation_matrix(width, height, degrees):
    """cv2.getRotationMatrix2D((width / 2, height / 2), degrees, 1): centre rounded to fp32."""
    cx = float(np.float32(width / 2))
    cy = float(np.float32(height / 2))
    a = degrees * math.pi / 180
    al = math.cos(a)
    be = math.sin(a)
    return [[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]]


def _u8_batch(images) -> torch.Tensor:
    if isinstance(images, torch.Tensor):
        t = images
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(images, dtype=np.uint8)))
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError("images must be a uint8 (N, H, W, 3) batch, got {} {}".format(t.dtype, tuple(t.shape)))
    return t.to(device="cuda", non_blocking=True).contiguous()


class DeviceImageAugmenter:
    def __init__(self, hsv_pert_tuples=None, rotation_tuple=None, horizontal_flip_prob=None, translation_tuple=None):
        # the reference's attribute names: (low, high) per HSV channel, (low, high) degrees, a probability,
        # and (t0, t1) for whole-pixel shifts drawn from [-t0, t1]; None switches a step off
        self.hsv_pert_tuples = hsv_pert_tuples
        self.rotation_tuple = rotation_tuple
        self.horizontal_flip_prob = horizontal_flip_prob
        self.translation_tuple = translation_tuple

    def draw_one(self, rng=np.random):
        """The draws of one ``augment`` call, in its order."""
        p = {}
        if self.hsv_pert_tuples is not None:
            hue = rng.uniform(*self.hsv_pert_tuples[0])
            sat = rng.uniform(*self.hsv_pert_tuples[1])
            val = rng.uniform(*self.hsv_pert_tuples[2])
            p["hsv"] = (hue, sat, val)
        if self.rotation_tuple is not None:
            p["rotation"] = rng.uniform(*self.rotation_tuple)
        if self.translation_tuple is not None:
            # np.random.random_integers(low, high) is randint(low, high + 1)
            lo, hi = -self.translation_tuple[0], self.translation_tuple[1] + 1
            row_trans = rng.randint(lo, hi)
            col_trans = rng.randint(lo, hi)
            p["translation"] = (row_trans, col_trans)
        if self.horizontal_flip_prob is not None:
            p["flip"] = bool(rng.uniform() < self.horizontal_flip_prob)
        return p

    def draw(self, n, rng=np.random):
        return [self.draw_one(rng) for _ in range(n)]

    @staticmethod
    def pack(params, height, width):
        """The device table (PARAMS_DTYPE, one record per image) for images of height x width."""
        tab = np.zeros(len(params), dtype=PARAMS_DTYPE)
        for i, p in enumerate(params):
            flags = 0
            hsv = p.get("hsv")
            if hsv is not None:
                f = np.asarray(hsv, dtype=np.float32).reshape(3)
                if not np.all(np.isfinite(f)):
                    raise ValueError("HSV factors must be finite, got {}".format(hsv))
                tab["hsv"][i] = f
                flags |= FLAG_HSV
            rot = p.get("rotation")
            if rot is not None:
                if not math.isfinite(rot):
                    raise ValueError("rotation must be finite, got {}".format(rot))
                tab["m"][i] = invert_affine(rotation_matrix(width, height, float(rot)))
                flags |= FLAG_ROTATE
            tr = p.get("translation")
            if tr is not None:
                row_trans, col_trans = tr
                if int(row_trans) != row_trans or int(col_trans) != col_trans:
                    raise ValueError("translations must be whole pixels, got {}".format(tr))
                if abs(int(row_trans)) > _INT_MAX or abs(int(col_trans)) > _INT_MAX:
                    raise ValueError("translation out of range: {}".format(tr))
                tab["tx"][i] = int(row_trans)  # the reference's quirk: row_trans moves columns
                tab["ty"][i] = int(col_trans)
            if p.get("flip"):
                flags |= FLAG_FLIP
            tab["flags"][i] = flags
        return tab

    def _table(self, params, n, height, width, device):
        if len(params) != n:
            raise ValueError("{} parameter sets for {} images".format(len(params), n))
        tab = self.pack(params, height, width)
        return torch.from_numpy(tab.view(np.uint8).reshape(n, PARAMS_DTYPE.itemsize)).to(device)

    def augment_batch(self, images, rng=np.random, params=None):
        """uint8 (N, H, W, 3) -> augmented uint8 (N, H, W, 3) on the GPU."""
        x = _u8_batch(images)
        N, H, W, C = x.shape
        if params is None:
            params = self.draw(N, rng)
        tab = self._table(params, N, H, W, x.device)
        out = torch.empty_like(x)
        lib.dk_augment_u8(x.data_ptr(), N, H, W, C, 0, H, W, tab.data_ptr(), out.data_ptr(), stream_handle())
        self._keep = (x, tab)  # alive until the stream has run the kernel
        return out

    def augment_crop_to_nchw(self, x, crop, rows, cols, params, shift=128.0):
        """Crop + augment + cast in one kernel: x uint8 (N, H, W, 3) on the GPU, crop a device int32
        (N, 2) tensor of (row, col) offsets or None, -> fp32 (N, 3, rows, cols) minus shift."""
        N, H, W, C = x.shape
        tab = self._table(params, N, rows, cols, x.device)
        out = torch.empty((N, C, rows, cols), dtype=torch.float32, device=x.device)
        lib.dk_augment_u8_to_nchw_f32(x.data_ptr(), N, H, W, C, crop.data_ptr() if crop is not None else 0, rows, cols,
                                      tab.data_ptr(), float(shift), out.data_ptr(), stream_handle())
        self._keep = (x, crop, tab)
        return out
