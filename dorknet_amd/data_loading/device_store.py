"""Device-resident image store.

Reference: ``ImageDataLoader`` (data_loading/image_data_loader.py:9-122) keeps a list of file paths
and decodes every image again each time it is drawn (``cv2.imread`` in
image_preprocessor.py:41-44).  ``DeviceImageStore`` decodes each image once and keeps the decoded
uint8 HWC pixels of the whole set in HBM, images of differing sizes back to back in one buffer:

- ``data``: one uint8 device tensor, the images one after the other, each ``H_i * W_i * C`` bytes
  (C fixed per store, 1 <= C <= 4);
- ``table``: one record per image, ``RECORD_DTYPE`` = (int64 byte offset, int32 H, int32 W), the
  ``dk_store_image`` of include/dorknet_hip.h, on the device.

``DeviceImageDataLoader`` (device_loader.py) turns index lists over the store into network-ready
batches.  The store is packed in chunks through one host staging buffer, so the host never holds
a second copy of the set.

- ``DeviceImageStore.from_arrays(images, labels, class_names=None)``: ``images`` a sequence of
  uint8 ``(H_i, W_i, C)`` arrays of any sizes, ``labels`` one integer each.
- ``DeviceImageStore.from_folder(base_folder, decoder=None)``: the reference's directory layout
  ``<base>/<class>/images/<file>`` (image_data_loader.py:27-32), labels numbered by sorted class
  name (:29).  ``decoder`` maps a path to a uint8 HWC array; the default is ``cv2.imread`` (BGR,
  as the reference reads), imported when first needed.  Files of a class are taken in sorted
  order (the reference takes ``os.listdir`` order, which is not reproducible).
- ``len(store)``, ``.classes`` (their number), ``.class_names``, ``.labels`` (int32, host),
  ``.labels_device``, ``.shapes`` (int32 (n, 2): H, W), ``.channels``, ``.nbytes`` (of the pixels).
- ``image(i)``: one image copied back to the host, for tests and debugging.

Both constructors take ``device="cuda"``; ``device="cpu"`` builds the same store in host memory,
which serves ``DeviceImageDataLoader.plan_batch`` (the index streams and draws) but no kernel.
"""
from __future__ import annotations

import os

import numpy as np
import torch

# one record per image, the layout of dk_store_image in include/dorknet_hip.h
RECORD_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])
CHUNK_BYTES = 64 << 20  # the host staging buffer
_INT_MAX = 2 ** 31 - 1


def records(shapes, channels):
    """The record table (RECORD_DTYPE) of images of `shapes` ((n, 2): H, W) packed back to back."""
    shapes = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
    sizes = shapes[:, 0] * shapes[:, 1] * int(channels)
    tab = np.zeros(len(shapes), dtype=RECORD_DTYPE)
    tab["offset"][1:] = np.cumsum(sizes)[:-1]
    tab["h"], tab["w"] = shapes[:, 0], shapes[:, 1]
    return tab


def table_to_device(tab, device="cuda"):
    return torch.from_numpy(np.ascontiguousarray(tab).view(np.uint8).reshape(len(tab), tab.dtype.itemsize)).to(device)


def _check_image(im, channels, what):
    im = np.asarray(im)
    if im.dtype != np.uint8 or im.ndim != 3 or not 1 <= im.shape[2] <= 4 or im.shape[0] < 1 or im.shape[1] < 1:
        raise ValueError("{} must be a uint8 (H, W, C) array with H, W >= 1 and 1 <= C <= 4, got {} {}".format(
            what, im.dtype, im.shape))
    if channels is not None and im.shape[2] != channels:
        raise ValueError("{} has {} channels, the store has {}".format(what, im.shape[2], channels))
    if im.shape[0] > _INT_MAX or im.shape[1] > _INT_MAX:
        raise ValueError("{} is too large: {}".format(what, im.shape))
    return im


class _Packer:
    """Appends images to a growing uint8 device buffer through one host staging buffer."""

    def __init__(self, capacity, chunk_bytes, device):
        self.device = device
        self.data = torch.empty(max(int(capacity), 1), dtype=torch.uint8, device=device)
        self.used = 0
        self.chunk = np.empty(max(min(int(chunk_bytes), self.data.numel()), 1), dtype=np.uint8)
        self.fill = 0

    def _reserve(self, nbytes):
        need = self.used + nbytes
        if need > self.data.numel():
            grown = torch.empty(max(need, int(self.data.numel() * 1.5)), dtype=torch.uint8, device=self.device)
            grown[:self.used].copy_(self.data[:self.used])
            self.data = grown

    def _upload(self, host):
        n = host.size
        self._reserve(n)
        self.data[self.used:self.used + n].copy_(torch.from_numpy(host))  # pageable: done when it returns
        self.used += n

    def flush(self):
        if self.fill:
            self._upload(self.chunk[:self.fill])
            self.fill = 0

    def add(self, im):
        flat = np.ascontiguousarray(im).reshape(-1)
        if flat.size > self.chunk.size - self.fill:
            self.flush()
        if flat.size > self.chunk.size:
            self._upload(flat)
        else:
            self.chunk[self.fill:self.fill + flat.size] = flat
            self.fill += flat.size


def _default_decoder():
    try:
        import cv2
    except ImportError as e:
        raise ImportError("DeviceImageStore.from_folder needs OpenCV (cv2) to decode image files and it is not "
                          "installed; pass decoder=, a function from a path to a uint8 (H, W, C) array") from e
    return cv2.imread


class DeviceImageStore:
    def __init__(self, data, shapes, channels, labels, class_names=None):
        """`data`: uint8 device tensor holding the images of `shapes` back to back (its first
        sum(H * W * channels) bytes).  Use from_arrays / from_folder."""
        self.shapes = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(-1, 2))
        self.channels = int(channels)
        if len(self.shapes) < 1:
            raise ValueError("an image store needs at least one image")
        if len(self.shapes) > _INT_MAX:
            raise ValueError("too many images for 32-bit image indices: {}".format(len(self.shapes)))
        self.records = records(self.shapes, self.channels)
        last = self.records[-1]
        self.nbytes = int(last["offset"]) + int(last["h"]) * int(last["w"]) * self.channels
        if data.dtype != torch.uint8 or data.dim() != 1 or data.numel() < self.nbytes:
            raise ValueError("data must be a flat uint8 tensor of at least {} bytes".format(self.nbytes))
        self.data = data
        self.labels = np.ascontiguousarray(np.asarray(labels, dtype=np.int32).reshape(-1))
        if len(self.labels) != len(self.shapes):
            raise ValueError("{} labels for {} images".format(len(self.labels), len(self.shapes)))
        if class_names is None:
            class_names = [str(c) for c in range(int(self.labels.max()) + 1 if self.labels.max() >= 0 else 1)]
        self.class_names = list(class_names)
        self.classes = len(self.class_names)
        self.table = table_to_device(self.records, data.device)
        self.labels_device = torch.from_numpy(self.labels).to(data.device)

    def __len__(self):
        return len(self.shapes)

    @classmethod
    def _pack(cls, images, count_hint, capacity, chunk_bytes, device):
        packer, shapes, channels = None, [], None
        for i, im in enumerate(images):
            im = _check_image(im, channels, "image {}".format(i))
            channels = im.shape[2]
            if packer is None:
                packer = _Packer(capacity if capacity else im.size * max(count_hint, 1), chunk_bytes, device)
            packer.add(im)
            shapes.append(im.shape[:2])
        if packer is None:
            raise ValueError("an image store needs at least one image")
        packer.flush()
        return packer.data, shapes, channels

    @classmethod
    def from_arrays(cls, images, labels, class_names=None, chunk_bytes=CHUNK_BYTES, device="cuda"):
        capacity = 0
        if all(hasattr(im, "shape") and hasattr(im, "dtype") for im in images):
            capacity = sum(int(np.prod(im.shape, dtype=np.int64)) for im in images)  # exact: no regrowth
        data, shapes, channels = cls._pack(images, len(images), capacity, chunk_bytes, device)
        return cls(data, shapes, channels, labels, class_names)

    @classmethod
    def from_folder(cls, base_folder, decoder=None, capacity_bytes=None, chunk_bytes=CHUNK_BYTES, device="cuda"):
        """capacity_bytes: the decoded size of the set if known (the buffer then never regrows;
        otherwise it starts from the first image's size times the file count and grows by 1.5x)."""
        if decoder is None:
            decoder = _default_decoder()
        class_names = sorted(c for c in os.listdir(base_folder) if os.path.isdir(os.path.join(base_folder, c)))
        paths, labels = [], []
        for num, name in enumerate(class_names):
            folder = os.path.join(base_folder, name, "images")
            for f in sorted(os.listdir(folder)):
                paths.append(os.path.join(folder, f))
                labels.append(num)
        if not paths:
            raise ValueError("no images under {}".format(base_folder))

        def decoded():
            for p in paths:
                im = decoder(p)
                if im is None:  # cv2.imread's way of failing
                    raise ValueError("could not decode {}".format(p))
                yield im

        data, shapes, channels = cls._pack(decoded(), len(paths), capacity_bytes or 0, chunk_bytes, device)
        store = cls(data, shapes, channels, labels, class_names)
        store.paths = paths
        return store

    def image(self, i):
        """Image i copied back to the host, uint8 (H, W, C)."""
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError("image {} of a store of {}".format(i, len(self)))
        r = self.records[i]
        h, w = int(r["h"]), int(r["w"])
        off = int(r["offset"])
        return self.data[off:off + h * w * self.channels].cpu().numpy().reshape(h, w, self.channels)
