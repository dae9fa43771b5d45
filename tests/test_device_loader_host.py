"""The host side of DeviceImageDataLoader, without a GPU: plan_batch against a
restatement of the reference's get_batch_list and load_batch (data_loading/image_data_loader.py:71-112,
with preprocess_image's draws, image_preprocessor.py:18-34) driven by the same RandomState -- the
class-balanced and index streams over classes of unequal size across several wraps of every cycle,
shuffle_indices, the draw order with and without mixup and with the augmenter, the pairing of the two
mixup batches -- and DeviceImageStore.from_folder on a tree of .npy files.  The stores live in host
memory (device="cpu"): nothing here launches a kernel."""
import itertools
import os

import numpy as np
import pytest

from tests import _augment_ref as ref

LABELS = [2, 0, 2, 1, 0, 2, 2, 0, 2]   # 3, 1 and 5 images of classes 0, 1, 2, interleaved
HSV = ((0.9, 1.1), (0.5, 2), (0.5, 2))
AUG = dict(hsv_pert_tuples=HSV, rotation_tuple=(-15, 15), horizontal_flip_prob=0.5, translation_tuple=(4, 6))


def _store(labels=LABELS):
    from dorknet_amd.data_loading.device_store import DeviceImageStore
    rng = np.random.RandomState(0)
    ims = [rng.randint(0, 256, size=(2 + i % 3, 3 + i % 2, 3)).astype(np.uint8) for i in range(len(labels))]
    return DeviceImageStore.from_arrays(ims, labels, device="cpu"), ims


def _preprocessor(crop_mode, augment=False):
    from dorknet_amd.data_loading.device_augmentation import DeviceImageAugmenter
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    return DeviceImagePreprocessor((8, 6), crop_mode=crop_mode, precrop_size=(11, 13),
                                   image_augmenter=DeviceImageAugmenter(**AUG) if augment else None,
                                   apply_augmenter=augment)


class RefLoader:
    """image_data_loader.py:33-38 and :71-112 with store indices in place of paths and the draws of
    preprocess_image in place of the image work; the class cycle in sorted class order."""

    def __init__(self, labels, batch_size, class_balance, mixup, crop_mode, augment, rng):
        self.labels, self.batch_size, self.class_balance, self.mixup = labels, batch_size, class_balance, mixup
        self.crop_mode, self.augment, self.rng = crop_mode, augment, rng
        by_class = {c: [i for i, l in enumerate(labels) if l == c] for c in sorted(set(labels))}
        self.class_cycle = itertools.cycle([(c, itertools.cycle(p)) for c, p in by_class.items()])
        self.index_cycle = itertools.cycle(range(len(labels)))

    def shuffle_indices(self):
        self.index_cycle = itertools.cycle(list(self.rng.permutation(len(self.labels))))

    def get_batch_list(self):
        X, y = [], []
        for _ in range(self.batch_size):
            if self.class_balance:
                c, cycle = next(self.class_cycle)
                y.append(c)
                X.append(next(cycle))
            else:
                i = next(self.index_cycle)
                y.append(self.labels[i])
                X.append(i)
        return X, y

    def preprocess_image(self):
        """(row, col, augmenter draws): image_size (8, 6) of a resize to (11, 13) = 13 rows, 11 columns."""
        if self.crop_mode == "random":
            r = self.rng.randint(0, 13 - 8)
            c = self.rng.randint(0, 11 - 6)
        elif self.crop_mode == "center":
            r, c = int((13 - 8) / 2), int((11 - 6) / 2)
        else:
            r, c = 0, 0
        p = ref.draw_transcription(self.rng, HSV, (-15, 15), 0.5, (4, 6)) if self.augment else None
        return r, c, p

    def load_batch(self):
        X, y = self.get_batch_list()
        draws = [self.preprocess_image() for _ in X]
        if self.mixup is None:
            return (X, y, draws), None, None
        prop = self.rng.uniform(*self.mixup)
        Xm, ym = self.get_batch_list()
        draws_m = [self.preprocess_image() for _ in Xm]
        return (X, y, draws), (Xm, ym, draws_m), prop


def _same_half(half, want):
    X, y, draws = want
    assert half.indices.dtype == np.int32 and half.labels.dtype == np.int32 and half.table.dtype == np.int32
    assert half.indices.tolist() == X and half.labels.tolist() == y
    assert half.table.tolist() == [[i, r, c] for i, (r, c, _) in zip(X, draws)]
    if draws[0][2] is None:
        assert half.augment is None
    else:
        assert half.augment == [p for _, _, p in draws]


def _same_plan(plan, want):
    a, b, prop = want
    _same_half(plan.a, a)
    if b is None:
        assert plan.b is None and plan.prop is None
    else:
        _same_half(plan.b, b)
        assert plan.prop == prop


@pytest.mark.parametrize("class_balance", [True, False])
@pytest.mark.parametrize("mixup", [None, (0.1, 0.4)])
@pytest.mark.parametrize("crop_mode,augment", [("random", False), ("random", True), ("center", True), (None, False)])
def test_plan_batch_follows_the_reference_streams_and_draws(class_balance, mixup, crop_mode, augment):
    from dorknet_amd.data_loading.device_loader import DeviceImageDataLoader
    store, _ = _store()
    loader = DeviceImageDataLoader(store, 4, _preprocessor(crop_mode, augment), class_balance=class_balance,
                                   mixup_range_tuple=mixup, rng=np.random.RandomState(5))
    want = RefLoader(LABELS, 4, class_balance, mixup, crop_mode, augment, np.random.RandomState(5))
    # 9 rounds of 4 (8 with mixup) images: the index cycle (9), the class cycle (3) and the largest class's
    # cycle (5 images, one in three draws) all wrap more than once
    for _ in range(9):
        _same_plan(loader.plan_batch(), want.load_batch())
    if not class_balance:
        loader.shuffle_indices()
        want.shuffle_indices()
        seen = []
        for _ in range(5):
            plan, w = loader.plan_batch(), want.load_batch()
            _same_plan(plan, w)
            seen += plan.a.indices.tolist() + (plan.b.indices.tolist() if mixup else [])
        assert sorted(seen[:9]) == list(range(9)) and seen[:9] != list(range(9)) and seen[9:18] == seen[:9]


def test_balanced_stream_visits_classes_in_turn():
    from dorknet_amd.data_loading.device_loader import DeviceImageDataLoader
    store, _ = _store()
    loader = DeviceImageDataLoader(store, 6, _preprocessor(None), rng=np.random.RandomState(0))
    first, second = loader.plan_batch().a, loader.plan_batch().a
    assert first.labels.tolist() == [0, 1, 2, 0, 1, 2] and second.labels.tolist() == [0, 1, 2, 0, 1, 2]
    assert first.indices.tolist() == [1, 3, 0, 4, 3, 2] and second.indices.tolist() == [7, 3, 5, 1, 3, 6]
    loader.stop_thread()  # there is no thread: a no-op


def test_mixup_pairs_consecutive_batches_of_one_stream():
    """Batch B continues the stream where batch A stopped, and the proportion is drawn between them."""
    from dorknet_amd.data_loading.device_loader import DeviceImageDataLoader
    store, _ = _store()
    loader = DeviceImageDataLoader(store, 3, _preprocessor("random"), class_balance=False,
                                   mixup_range_tuple=(0.2, 0.3), rng=np.random.RandomState(3))
    plan = loader.plan_batch()
    assert plan.a.indices.tolist() == [0, 1, 2] and plan.b.indices.tolist() == [3, 4, 5]
    rng = np.random.RandomState(3)
    a = [(rng.randint(0, 5), rng.randint(0, 5)) for _ in range(3)]
    prop = rng.uniform(0.2, 0.3)
    b = [(rng.randint(0, 5), rng.randint(0, 5)) for _ in range(3)]
    assert plan.a.table[:, 1:].tolist() == [list(t) for t in a] and plan.b.table[:, 1:].tolist() == [list(t) for t in b]
    assert plan.prop == prop and 0.2 <= prop < 0.3


def test_store_tables_and_host_round_trip():
    from dorknet_amd.data_loading.device_store import RECORD_DTYPE
    store, ims = _store()
    assert len(store) == 9 and store.classes == 3 and store.channels == 3 and store.class_names == ["0", "1", "2"]
    assert store.labels.dtype == np.int32 and store.labels.tolist() == LABELS
    assert store.shapes.tolist() == [list(im.shape[:2]) for im in ims]
    assert store.nbytes == sum(im.size for im in ims) == store.data.numel()
    assert RECORD_DTYPE.itemsize == 16
    offs = np.cumsum([0] + [im.size for im in ims])[:-1]
    assert store.records["offset"].tolist() == offs.tolist() and store.records["offset"].dtype == np.int64
    assert tuple(store.table.shape) == (9, 16)
    for i, im in enumerate(ims):
        assert np.array_equal(store.image(i), im)


def test_store_packs_in_chunks():
    """A staging buffer smaller than the set, and smaller than one image, packs the same bytes."""
    from dorknet_amd.data_loading.device_store import DeviceImageStore
    _, ims = _store()
    for chunk in (1, 20, 40, 1 << 20):
        store = DeviceImageStore.from_arrays(ims, LABELS, chunk_bytes=chunk, device="cpu")
        assert np.array_equal(store.data.numpy()[:store.nbytes], np.concatenate([im.reshape(-1) for im in ims]))


def test_store_refuses_bad_images():
    from dorknet_amd.data_loading.device_store import DeviceImageStore
    ok = np.zeros((2, 2, 3), np.uint8)
    for bad in (np.zeros((2, 2, 3), np.float32), np.zeros((2, 2), np.uint8), np.zeros((2, 2, 5), np.uint8),
                np.zeros((0, 2, 3), np.uint8), np.zeros((2, 2, 1), np.uint8)):
        with pytest.raises(ValueError):
            DeviceImageStore.from_arrays([ok, bad], [0, 0], device="cpu")
    with pytest.raises(ValueError):
        DeviceImageStore.from_arrays([ok], [0, 1], device="cpu")
    with pytest.raises(ValueError):
        DeviceImageStore.from_arrays([], [], device="cpu")


def test_loader_argument_checks():
    import torch
    from dorknet_amd.data_loading.device_loader import DeviceImageDataLoader
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    store, _ = _store()
    with pytest.raises(ValueError):
        DeviceImageDataLoader(store, 0, _preprocessor(None))
    with pytest.raises(ValueError):
        DeviceImageDataLoader(store, 2, _preprocessor(None), out_dtype=torch.float16)
    with pytest.raises(ValueError):  # a crop larger than the pre-crop
        DeviceImageDataLoader(store, 2, DeviceImagePreprocessor((8, 8), crop_mode="center", precrop_size=(7, 9)))
    loader = DeviceImageDataLoader(store, 2, _preprocessor(None))
    with pytest.raises(RuntimeError, match="on the GPU"):  # a host store plans batches but produces none
        next(loader.pull_batch(1))


def test_from_folder_numbers_labels_by_sorted_class_name(tmp_path):
    from dorknet_amd.data_loading.device_store import DeviceImageStore
    rng = np.random.RandomState(1)
    want = {}
    for name, count in (("terrier", 2), ("beagle", 3), ("collie", 1)):   # created out of order
        os.makedirs(tmp_path / name / "images")
        for k in range(count):
            im = rng.randint(0, 256, size=(3 + k, 4 + len(name) % 3, 3)).astype(np.uint8)
            np.save(tmp_path / name / "images" / "im{}.npy".format(k), im)
            want[(name, k)] = im
    (tmp_path / "notes.txt").write_text("not a class")   # only directories are classes (:27-28)
    store = DeviceImageStore.from_folder(str(tmp_path), decoder=np.load, device="cpu")
    assert store.class_names == ["beagle", "collie", "terrier"] and store.classes == 3
    assert store.labels.tolist() == [0, 0, 0, 1, 2, 2] and len(store) == 6
    order = [("beagle", 0), ("beagle", 1), ("beagle", 2), ("collie", 0), ("terrier", 0), ("terrier", 1)]
    for i, key in enumerate(order):
        assert np.array_equal(store.image(i), want[key])
        assert store.paths[i] == str(tmp_path / key[0] / "images" / "im{}.npy".format(key[1]))


def test_from_folder_without_cv2_needs_a_decoder(tmp_path, monkeypatch):
    import sys
    from dorknet_amd.data_loading.device_store import DeviceImageStore
    monkeypatch.setitem(sys.modules, "cv2", None)   # `import cv2` raises ImportError, installed or not
    os.makedirs(tmp_path / "a" / "images")
    np.save(tmp_path / "a" / "images" / "x.npy", np.zeros((2, 2, 3), np.uint8))
    with pytest.raises(ImportError, match="decoder="):
        DeviceImageStore.from_folder(str(tmp_path), device="cpu")
