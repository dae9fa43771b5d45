"""A device-resident image store and its batch loader in front of a few training steps and an
evaluation: synthetic uint8 BGR images of mixed sizes (standing in for a decoded ImageNet folder, whose
images never share a size) are packed once into HBM; DeviceImageDataLoader -- the reference's
ImageDataLoader interface (data_loading/image_data_loader.py:9-122) -- then turns class-balanced index
lists into mixed-up, network-ready batches with one kernel per batch pair, ResNet-18-depsep trains on
them and net.evaluate runs over a second, centre-cropped loader.  A real set is loaded with
DeviceImageStore.from_folder(base_folder) in place of from_arrays.

    python examples/device_loader.py --batch 16 --steps 4
    python examples/device_loader.py --batch 16 --steps 4 --bf16      # bf16 channels-last batches
    python examples/device_loader.py --batch 16 --steps 4 --augment   # the augmenter applied
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.resnet18_depsep import ResNet18  # noqa: E402


def synthetic_images(count, num_classes, seed=0):
    """Noisy waves as uint8 BGR images of sizes drawn around 375 x 500, portrait and landscape, and their labels."""
    import numpy as np
    rng = np.random.RandomState(seed)
    ims, labels = [], []
    for n in range(count):
        h, w = rng.randint(300, 451), rng.randint(400, 601)
        if rng.uniform() < 0.3:
            h, w = w, h
        ys, xs = np.mgrid[0:h, 0:w]
        im = np.empty((h, w, 3), np.uint8)
        for c in range(3):
            fy, fx, ph = rng.uniform(0.01, 0.05), rng.uniform(0.01, 0.05), rng.uniform(0, 6.28)
            wave = 127.5 + 80 * np.sin(fy * ys + fx * xs + ph) + rng.uniform(-40, 40, size=(h, w))
            im[:, :, c] = np.clip(wave, 0, 255).astype(np.uint8)
        ims.append(im)
        labels.append(n % num_classes)
    return ims, labels


def main():
    import numpy as np
    import torch
    from dorknet_amd.data_loading.device_augmentation import DeviceImageAugmenter
    from dorknet_amd.data_loading.device_loader import DeviceImageDataLoader
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    from dorknet_amd.data_loading.device_store import DeviceImageStore
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=225)
    ap.add_argument("--bf16", action="store_true", help="bf16 channels-last batches straight from the loader")
    ap.add_argument("--augment", action="store_true", help="apply the flagship script's augmenter")
    args = ap.parse_args()
    np.random.seed(0)
    classes = 120
    ims, labels = synthetic_images(args.images, classes)
    store = DeviceImageStore.from_arrays(ims, labels, class_names=["class{:03d}".format(c) for c in range(classes)])
    print("store: {} images, {} to {} rows, {} to {} columns, {:.1f} MB in HBM".format(
        len(store), store.shapes[:, 0].min(), store.shapes[:, 0].max(), store.shapes[:, 1].min(),
        store.shapes[:, 1].max(), store.nbytes / 1e6))
    dtype = torch.bfloat16 if args.bf16 else torch.float32
    augmenter = DeviceImageAugmenter(hsv_pert_tuples=((0.9, 1.1), (0.5, 2), (0.5, 2)), rotation_tuple=(-15, 15),
                                     horizontal_flip_prob=0.5)
    train_pp = DeviceImagePreprocessor((args.size, args.size), crop_mode="random", image_augmenter=augmenter,
                                       apply_augmenter=args.augment)
    train = DeviceImageDataLoader(store, args.batch, train_pp, class_balance=True, mixup_range_tuple=(0.0, 0.4),
                                  out_dtype=dtype)
    net = ResNet18("device_loader")
    net.to_gpu()
    sgd = SGDMomentum(net, 0.05 * (args.batch / 200.0), 0.9)
    for i, (X, y, y_one_hot) in enumerate(train.pull_batch(args.steps)):
        loss, _ = net.forward(X, y_one_hot)
        net.backward()
        sgd.update_weights()
        print("step {}: X {} {}, loss {:.5f}".format(i, tuple(X.shape), str(X.dtype).replace("torch.", ""), float(loss)))
    train.stop_thread()
    val_pp = DeviceImagePreprocessor((args.size, args.size), crop_mode="center")
    val = DeviceImageDataLoader(store, args.batch, val_pp, class_balance=False, out_dtype=dtype)
    print(net.evaluate(val, top=(1, 5)))


if __name__ == "__main__":
    main()
