"""Class activation maps on the GPU.

Reference: ``returnCAM`` and ``show_cam_on_image`` of examples/imagenet_dogs_225_resnet_18_depsep_CAM.py
(:13-49) take one image at a time to the host: the ``res8`` feature map times one row of the dense
weights per class, ``cv2.resize`` to the image size, clip / shift / scale, ``COLORMAP_JET`` added onto
the image, divided by the maximum, uint8.  Here the same arithmetic runs for a whole batch and all
requested classes in one HIP launch (dk_cam_f32 / dk_cam_bf16 in dorknet_amd/csrc/cam.hip, one workgroup
per map), and the arg-sort that picks the classes in another (dk_topk_rows_f32).

- ``top_classes(scores, k=3)``: ``np.argsort(scores)[::-1][:k]`` per row, as an int32 (N, k) device tensor.
- ``top_classes_with_scores(scores, k=5)``: the same indices and the scores at them (dk_topk_rows_vals_f32;
  ``FeedForwardNetwork.predict``).
- ``class_activation_maps(features, dense_weights, class_idx, images=None, out_size=None, shift=128.0,
  want_masks=True)`` -> ``(masks | None, overlays | None)``: fp32 (N, K, H, W) masks (the reference's
  ``cam_img``) and uint8 (N, K, H, W, 3) BGR overlays, both on the GPU.
- ``FeedForwardNetwork.class_activation_maps`` runs the network and calls both.

The cv2 calls are restated from OpenCV 4.3 and the colour table from its definition
(tests/_cam_ref.py pins the kernel bit for bit); cv2 is not installed to compare against, so agreement
with cv2's own ``resize`` and ``COLORMAP_JET`` is unpinned.
"""
from __future__ import annotations

import torch

from ._hip import lib, stream_handle
from ._tensor import BF16, F32, is_nhwc, to_nhwc

MAX_MAP = 1024   # h * w positions one workgroup keeps in LDS
MAX_TOP = 16


def top_classes(scores, k=3) -> torch.Tensor:
    """The k best classes of each row of `scores` (N, classes), best first; of equal scores the higher
    index comes first, as ``np.argsort(scores)[::-1]`` orders them.  int32 (N, k) on the GPU."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
        raise ValueError("scores must be a 2-D (N, classes) tensor, got {}".format(
            tuple(scores.shape) if hasattr(scores, "shape") else type(scores)))
    n, classes = scores.shape
    k = int(k)
    if n < 1 or not 1 <= k <= min(classes, MAX_TOP):
        raise ValueError("top_classes needs N >= 1 and 1 <= k <= min(classes, {}), got N = {}, classes = {}, "
                         "k = {}".format(MAX_TOP, n, classes, k))
    s = scores.to(device="cuda", dtype=F32).contiguous()
    out = torch.empty((n, k), dtype=torch.int32, device=s.device)
    lib.dk_topk_rows_f32(s.data_ptr(), n, classes, k, out.data_ptr(), stream_handle())
    return out


def top_classes_with_scores(scores, k=5):
    """``top_classes`` plus the k scores themselves (dk_topk_rows_vals_f32): (int32 (N, k), fp32 (N, k)),
    both on the GPU, ``values == scores.gather(1, idx)``."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
        raise ValueError("scores must be a 2-D (N, classes) tensor, got {}".format(
            tuple(scores.shape) if hasattr(scores, "shape") else type(scores)))
    n, classes = scores.shape
    k = int(k)
    if n < 1 or not 1 <= k <= min(classes, MAX_TOP):
        raise ValueError("top_classes_with_scores needs N >= 1 and 1 <= k <= min(classes, {}), got N = {}, "
                         "classes = {}, k = {}".format(MAX_TOP, n, classes, k))
    s = scores.to(device="cuda", dtype=F32).contiguous()
    idx = torch.empty((n, k), dtype=torch.int32, device=s.device)
    val = torch.empty((n, k), dtype=F32, device=s.device)
    lib.dk_topk_rows_vals_f32(s.data_ptr(), n, classes, k, idx.data_ptr(), val.data_ptr(), stream_handle())
    return idx, val


def class_activation_maps(features, dense_weights, class_idx, images=None, out_size=None, shift=128.0,
                          want_masks=True):
    """features: logical (N, C, h, w) with channels_last strides, fp32 or bf16, as every layer returns
    it (anything else is converted); dense_weights: the DenseLayer's fp32 (C, classes) array; class_idx:
    (N, K) integers; images: the network's fp32 (N, 3, H, W) input batch (B, G, R) or None; out_size:
    (H, W), by default the images'.  Without images out_size is required and only masks come back.
    Returns (masks fp32 (N, K, H, W) or None, overlays uint8 (N, K, H, W, 3) or None)."""
    for name, t, rank in (("features", features, 4), ("dense_weights", dense_weights, 2), ("class_idx", class_idx, 2)):
        if not isinstance(t, torch.Tensor) or t.dim() != rank:
            raise ValueError("{} must be a {}-D tensor, got {}".format(
                name, rank, tuple(t.shape) if hasattr(t, "shape") else type(t)))
    if features.dtype not in (F32, BF16):
        raise ValueError("features must be fp32 or bf16, got {}".format(features.dtype))
    n, c, h, w = features.shape
    if dense_weights.dtype != F32 or dense_weights.shape[0] != c or dense_weights.shape[1] < 1:
        raise ValueError("dense_weights must be fp32 ({}, classes), got {} {}".format(
            c, dense_weights.dtype, tuple(dense_weights.shape)))
    if class_idx.shape[0] != n or class_idx.shape[1] < 1 or class_idx.dtype.is_floating_point:
        raise ValueError("class_idx must be an integer ({}, K) tensor, got {} {}".format(
            n, class_idx.dtype, tuple(class_idx.shape)))
    if min(n, c, h, w) < 1 or h * w > MAX_MAP:
        raise ValueError("features need N, C, h, w >= 1 and h * w <= {}, got {}".format(MAX_MAP, tuple(features.shape)))
    if images is not None:
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[0] != n or images.shape[1] != 3 \
                or images.dtype != F32:
            raise ValueError("images must be an fp32 ({}, 3, H, W) tensor, got {} {}".format(
                n, getattr(images, "dtype", None), tuple(images.shape) if hasattr(images, "shape") else type(images)))
        if out_size is None:
            out_size = tuple(images.shape[2:])
        elif tuple(out_size) != tuple(images.shape[2:]):
            raise ValueError("out_size {} differs from the images' {}".format(tuple(out_size), tuple(images.shape[2:])))
    elif out_size is None:
        raise ValueError("without images an out_size (H, W) is required")
    if images is None and not want_masks:
        raise ValueError("nothing to compute: no images (so no overlays) and want_masks is False")
    H, W = (int(v) for v in out_size)
    if H < 1 or W < 1 or H * W > 2 ** 31 - 1 - 2048:
        raise ValueError("out_size must be (H, W) with 1 <= H * W <= 2^31 - 2049, got {}".format((H, W)))

    feat = features if features.is_cuda and is_nhwc(features) else to_nhwc(features)
    wts = dense_weights.to(device=feat.device).contiguous()
    idx = class_idx.to(device=feat.device, dtype=torch.int32).contiguous()
    k = idx.shape[1]
    img = None if images is None else images.to(device=feat.device).contiguous()
    masks = torch.empty((n, k, H, W), dtype=F32, device=feat.device) if want_masks else None
    overlays = None if img is None else torch.empty((n, k, H, W, 3), dtype=torch.uint8, device=feat.device)
    entry = lib.dk_cam_bf16 if feat.dtype == BF16 else lib.dk_cam_f32
    entry(feat.data_ptr(), n, h, w, c, wts.data_ptr(), wts.shape[1], idx.data_ptr(), k,
          0 if img is None else img.data_ptr(), H, W, float(shift), 0 if masks is None else masks.data_ptr(),
          0 if overlays is None else overlays.data_ptr(), stream_handle())
    return masks, overlays
