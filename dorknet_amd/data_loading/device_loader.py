"""Batch loader over a device-resident image store.

Reference: ``ImageDataLoader`` (data_loading/image_data_loader.py:9-122) -- a thread that draws a
list of image paths (class-balanced or from an index cycle), has a pool of workers decode and
preprocess them with cv2, builds the one-hot labels, optionally draws a second batch and mixes the
two up, and queues ``(X_batch, y_batch, y_one_hot)`` triples for ``pull_batch``.

``DeviceImageDataLoader`` has that interface over a ``DeviceImageStore`` (device_store.py).  There
is no thread and no queue of prepared batches: a batch is produced on the current stream when it
is asked for, from the decoded pixels already in HBM, by one kernel that gathers the images,
resizes each from its own size (the crop window only), crops, casts, shifts by 128, mixes up and
writes the network's layout (dk_store_batch_nchw_f32 / dk_store_batch_nhwc_bf16), and one that
writes the (mixed) one-hot rows (dk_onehot_mixup_f32).  With ``apply_augmenter`` the cropped uint8
images of both batches are written first (dk_store_crop_u8), augmented in one launch
(dk_augment_u8) and then taken through the same two kernels as a dense store.

- ``DeviceImageDataLoader(store, batch_size, preprocessor, class_balance=True,
  mixup_range_tuple=None, out_dtype=torch.float32, rng=np.random)``: ``preprocessor`` is a
  ``DeviceImagePreprocessor``; its ``image_size``, ``precrop_size``, ``crop_mode`` and
  ``apply_augmenter`` mean what they mean in ``preprocess_batch``.  ``out_dtype`` fp32 gives X as
  NCHW (the reference's X_batch), bfloat16 a channels_last tensor of the same shape.
- ``pull_batch(num_steps)`` yields ``(X, y, y_one_hot)``: X on the GPU, y the int32 labels on the
  GPU, y_one_hot fp32.  With mixup the two mirrored batches come one after the other as the
  reference queues them (:111-112); the second of a pair that ``num_steps`` cuts off is the first
  of the next call, as it would wait in the reference's queue.  Iterating the loader itself gives
  ``len(store) // batch_size`` (at least one) batches, what ``test`` and ``evaluate`` take.
- ``plan_batch()``: the host side of one ``load_batch`` round -- indices, labels, crop offsets,
  augmentation draws and the mixup proportion -- as numpy tables, without touching the GPU;
  ``pull_batch`` uploads exactly these.
- ``shuffle_indices()`` replaces the index cycle by ``rng.permutation(len(store))`` (:66-68);
  ``stop_thread()`` does nothing (there is no thread).

Index streams as in ``get_batch_list`` (:71-86).  Class-balanced: the next class of a cycle over
the classes and that class's next image, both cycles persistent; otherwise the persistent index
cycle.  The class cycle runs in sorted class order (label order) and a class's images in store
order: the reference cycles in ``os.listdir`` order, which depends on the file system and is not
reproducible.  Classes without images are left out of the cycle.

Random draws, in the reference's order for one worker (with more workers the reference's order is
a race): batch A's per-image draws (crop row, crop column, then the augmenter's when applied), then
``rng.uniform(*mixup_range_tuple)``, then batch B's per-image draws.  The mixup factors are
``np.float32(prop)`` and ``np.float32(1 - prop)`` as in ``mixup_batches``.
"""
from __future__ import annotations

import itertools
from collections import deque

import numpy as np
import torch

from .device_store import records, table_to_device


class BatchHalf:
    """One batch of a plan: `indices` int32 (N,) into the store, `labels` int32 (N,), `table` int32
    (N, 3) of (image index, crop row, crop col), `augment` one DeviceImageAugmenter.draw_one record
    per image or None."""
    __slots__ = ("indices", "labels", "table", "augment")

    def __init__(self, indices, labels, table, augment):
        self.indices, self.labels, self.table, self.augment = indices, labels, table, augment


class BatchPlan:
    """`a`, and with mixup `b` (the partner batch) and `prop`; else b and prop are None."""
    __slots__ = ("a", "b", "prop")

    def __init__(self, a, b=None, prop=None):
        self.a, self.b, self.prop = a, b, prop


class DeviceImageDataLoader:
    def __init__(self, store, batch_size, preprocessor, class_balance=True, mixup_range_tuple=None,
                 out_dtype=torch.float32, rng=np.random):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1, got {}".format(batch_size))
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("out_dtype must be torch.float32 or torch.bfloat16, got {}".format(out_dtype))
        self.store = store
        self.batch_size = int(batch_size)
        self.preprocessor = preprocessor
        self.class_balance = bool(class_balance)
        self.mixup_range_tuple = mixup_range_tuple
        self.out_dtype = out_dtype
        self.rng = rng
        pp = preprocessor
        # cv2.resize takes (width, height); the crop is image_size[0] rows by image_size[1] columns
        if pp.crop_mode in ("random", "center"):
            self.target = (int(pp.precrop_size[1]), int(pp.precrop_size[0]))  # (TH, TW)
            self.window = (int(pp.image_size[0]), int(pp.image_size[1]))      # (OH, OW)
        else:
            self.target = (int(pp.image_size[1]), int(pp.image_size[0]))
            self.window = self.target
        if self.window[0] > self.target[0] or self.window[1] > self.target[1] or min(self.window) < 1:
            raise ValueError("crop {}x{} larger than the resized image {}x{}".format(*self.window, *self.target))
        self.augment = bool(getattr(pp, "apply_augmenter", False))
        if self.augment and store.channels != 3:
            raise ValueError("augmentation needs BGR images (C = 3), got C = {}".format(store.channels))
        by_class = [np.flatnonzero(store.labels == c) for c in range(store.classes)]
        self.class_cycle = itertools.cycle([(c, itertools.cycle(ix.tolist())) for c, ix in enumerate(by_class) if len(ix)])
        self.index_cycle = itertools.cycle(range(len(store)))
        self._queue = deque()
        self._dense = {}
        self._keep = None

    # -- the host side ---------------------------------------------------------------------------
    def stop_thread(self):
        """Nothing to stop: batches are produced on the current stream when pulled."""

    def shuffle_indices(self):
        self._queue.clear()  # the reference drops the batches already queued
        self.index_cycle = itertools.cycle(list(self.rng.permutation(len(self.store))))

    def _next_indices(self):
        if self.class_balance:
            return [next(cycle) for _, cycle in (next(self.class_cycle) for _ in range(self.batch_size))]
        return [int(next(self.index_cycle)) for _ in range(self.batch_size)]

    def _half(self, indices):
        pp, rng = self.preprocessor, self.rng
        table = np.zeros((len(indices), 3), dtype=np.int32)
        table[:, 0] = indices
        augment = None
        if self.augment:
            augment = []
            for i in range(len(indices)):  # preprocess_image's order: the crop's draws, then the augmenter's
                off = pp.crop_offsets(1, self.target, rng)
                if off is not None:
                    table[i, 1:] = off[0]
                augment.append(pp.image_augmenter.draw_one(rng))
        else:
            off = pp.crop_offsets(len(indices), self.target, rng)  # image by image: row, then column
            if off is not None:
                table[:, 1:] = off
        indices = np.asarray(indices, dtype=np.int32)
        return BatchHalf(indices, self.store.labels[indices], table, augment)

    def plan_batch(self):
        """One load_batch round on the host: a BatchPlan.  Touches no GPU."""
        a = self._half(self._next_indices())
        if self.mixup_range_tuple is None:
            return BatchPlan(a)
        prop = self.rng.uniform(*self.mixup_range_tuple)
        return BatchPlan(a, self._half(self._next_indices()), prop)

    # -- the device side -------------------------------------------------------------------------
    def _dense_store(self, m, device):
        """Record and batch tables of m cropped images as a dense store (copy mode)."""
        OH, OW = self.window
        d = self._dense.get(m)
        if d is None:
            tab = np.zeros((m, 3), dtype=np.int32)
            tab[:, 0] = np.arange(m)
            d = self._dense[m] = (table_to_device(records(np.tile([[OH, OW]], (m, 1)), 3), device),
                                  torch.from_numpy(tab).to(device))
        return d

    def _produce(self, plan):
        from .._hip import lib, stream_handle
        store = self.store
        if store.data.device.type != "cuda":
            raise RuntimeError("pull_batch needs the store on the GPU (it was built with device={!r})".format(
                str(store.data.device)))
        dev = store.data.device
        N, C = self.batch_size, store.channels
        (TH, TW), (OH, OW) = self.target, self.window
        mix = plan.b is not None
        halves = (plan.a, plan.b) if mix else (plan.a,)
        M = N * len(halves)
        # one upload: the batch tables, then the labels
        host = np.concatenate([h.table.reshape(-1) for h in halves] + [h.labels for h in halves]).astype(np.int32)
        # (through pinned memory and without blocking: a copy from pageable memory waits for the stream,
        # i.e. for the training step queued before this batch)
        up = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)
        tables, labels = up[:3 * M].view(M, 3), up[3 * M:]
        p = float(np.float32(plan.prop)) if mix else 0.0
        q = float(np.float32(1 - plan.prop)) if mix else 0.0
        stream = stream_handle()
        data, images, count, keep = store.data, store.table, len(store), [up]
        if self.augment:
            aug = self.preprocessor.image_augmenter
            crop = torch.empty((M, OH, OW, 3), dtype=torch.uint8, device=dev)
            lib.dk_store_crop_u8(data.data_ptr(), images.data_ptr(), count, C, tables.data_ptr(), M, TH, TW, OH, OW,
                                 crop.data_ptr(), stream)
            params = aug._table([r for h in halves for r in h.augment], M, OH, OW, dev)
            data = torch.empty_like(crop)
            lib.dk_augment_u8(crop.data_ptr(), M, OH, OW, 3, 0, OH, OW, params.data_ptr(), data.data_ptr(), stream)
            images, tables = self._dense_store(M, dev)
            keep += [crop, params, data]
            count, TH, TW = M, OH, OW
        bf16 = self.out_dtype == torch.bfloat16
        fmt = torch.channels_last if bf16 else torch.contiguous_format
        entry = lib.dk_store_batch_nhwc_bf16 if bf16 else lib.dk_store_batch_nchw_f32
        X = [torch.empty((N, C, OH, OW), dtype=self.out_dtype, device=dev, memory_format=fmt) for _ in halves]
        Y = [torch.empty((N, store.classes), dtype=torch.float32, device=dev) for _ in halves]
        entry(data.data_ptr(), images.data_ptr(), count, C, tables.data_ptr(), tables[N:].data_ptr() if mix else 0, N,
              TH, TW, OH, OW, 128.0, p, q, X[0].data_ptr(), X[1].data_ptr() if mix else 0, stream)
        lib.dk_onehot_mixup_f32(labels.data_ptr(), labels[N:].data_ptr() if mix else 0, N, store.classes, p, q,
                                Y[0].data_ptr(), Y[1].data_ptr() if mix else 0, stream)
        self._keep = keep  # alive until the stream has run the kernels
        return [(X[k], labels[k * N:(k + 1) * N], Y[k]) for k in range(len(halves))]

    def pull_batch(self, num_steps):
        for _ in range(int(num_steps)):
            if not self._queue:
                self._queue.extend(self._produce(self.plan_batch()))
            yield self._queue.popleft()

    def __iter__(self):
        return self.pull_batch(max(1, len(self.store) // self.batch_size))
