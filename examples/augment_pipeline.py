"""The whole device-side input pipeline in front of one training step: a synthetic uint8 BGR batch
(standing in for decoded images) is resized to the pre-crop size, cropped at random, augmented with
the flagship script's augmenter (reference: examples/imagenet_dogs_225_resnet_18_depsep.py:167-172 --
HSV perturbation 0.9-1.1 / 0.5-2 / 0.5-2, rotation +-15 degrees, flip 0.5) and cast to the fp32 NCHW
batch the network eats; two such batches are mixed up (image_data_loader.py:101-111) and
ResNet-18-depsep takes one SGD-momentum step on the result.  In the reference the augmenter's result is
dropped (image_preprocessor.py:33-34); apply_augmenter=True is what makes it count here.

    python examples/augment_pipeline.py --batch 16
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.resnet18_depsep import ResNet18  # noqa: E402


def synthetic_images(batch, height=300, width=400, num_classes=120, seed=0):
    """Smooth uint8 BGR images (so a rotation or a hue shift is visible in the statistics) and one-hot labels."""
    import numpy as np
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:height, 0:width]
    ims = np.empty((batch, height, width, 3), np.uint8)
    for n in range(batch):
        for c in range(3):
            fy, fx, ph = rng.uniform(0.01, 0.05), rng.uniform(0.01, 0.05), rng.uniform(0, 6.28)
            ims[n, :, :, c] = (127.5 + 120 * np.sin(fy * ys + fx * xs + ph)).astype(np.uint8)
    onehot = np.eye(num_classes, dtype=np.float32)[rng.randint(0, num_classes, batch)]
    return ims, onehot


def main():
    import numpy as np
    import torch
    from dorknet_amd._tensor import as_device
    from dorknet_amd.data_loading.device_augmentation import DeviceImageAugmenter
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor, mixup_batches
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=225)
    args = ap.parse_args()
    np.random.seed(0)
    augmenter = DeviceImageAugmenter(hsv_pert_tuples=((0.9, 1.1), (0.5, 2), (0.5, 2)), rotation_tuple=(-15, 15),
                                     horizontal_flip_prob=0.5)
    pre = DeviceImagePreprocessor((args.size, args.size), crop_mode="random", image_augmenter=augmenter,
                                  apply_augmenter=True)
    plain = DeviceImagePreprocessor((args.size, args.size), crop_mode="random", image_augmenter=augmenter)
    ims, y = synthetic_images(args.batch, seed=0)
    ims_m, y_m = synthetic_images(args.batch, seed=1)
    X = pre.preprocess_batch(ims)            # resize, then crop + augment + cast in one kernel
    X_m = pre.preprocess_batch(ims_m)
    X0 = plain.preprocess_batch(ims)          # the default: the augmenter has no effect
    print("batch {} -> {}: mean {:.2f} (augmented), {:.2f} (not augmented); {:.1f} % of the augmented pixels are border fill"
          .format(ims.shape, tuple(X.shape), float(X.mean()), float(X0.mean()), 100 * float((X == -128).all(dim=1).float().mean())))
    prop = np.random.uniform(0.0, 0.4)
    X_mix, X_mix_m, y_mix, y_mix_m = mixup_batches(X, X_m, as_device(y), as_device(y_m), prop)
    net = ResNet18("augmented")
    net.to_gpu()
    sgd = SGDMomentum(net, 0.05 * (args.batch / 200.0), 0.9)
    for name, (xb, yb) in (("mixed", (X_mix, y_mix)), ("mixed, mirrored", (X_mix_m, y_mix_m))):
        loss, _ = net.forward(xb, yb)
        net.backward()
        sgd.update_weights()
        torch.cuda.synchronize()
        print("one step on the {} batch (prop {:.3f}): loss {:.5f}".format(name, prop, float(loss)))


if __name__ == "__main__":
    main()
