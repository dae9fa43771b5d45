"""Evaluation of the ResNet-18-depsep model on the GPU (reference:
examples/imagenet_dogs_225_resnet_18_depsep_evaluate.py): decoded uint8 images are centre-cropped on the
device (DeviceImagePreprocessor, crop_mode="center"), ``net.predict`` gives the best five classes and
their scores for the whole batch (the reference arg-sorts one image's scores on the host), and
``net.evaluate`` runs a validation set through device-side counters and reports accuracy, top-5 accuracy,
loss and per-class accuracy with one read at the end (dorknet_amd/metrics.py).
The images are synthetic; the reference's cv2.putText of the best name into the image is left out.

    python examples/evaluate_resnet18.py                                   # fresh weights, synthetic images
    python examples/evaluate_resnet18.py --json net.json --h5 weights.h5   # a trained checkpoint
    python examples/evaluate_resnet18.py --bf16                            # bf16 activation storage
    python examples/evaluate_resnet18.py --names num_to_dog_name_map.json  # {"0": "Chihuahua", ...}

Without a checkpoint the network makes one training-mode forward pass over the first batch: the running
statistics that a test-mode forward pass reads exist only after the first batch.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.resnet18_depsep import ResNet18  # noqa: E402


def main():
    import numpy as np
    import torch
    from dorknet_amd._hip import require_gpu
    from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=60, help="images per batch (the reference evaluates 60 at a time)")
    ap.add_argument("--batches", type=int, default=3, help="synthetic validation batches")
    ap.add_argument("--size", type=int, default=225)
    ap.add_argument("--top", type=int, default=5)
    ap.add_argument("--show", type=int, default=4, help="images whose best classes are printed")
    ap.add_argument("--json", help="layer structure of a saved network (with --h5)")
    ap.add_argument("--h5", help="weights of a saved network (with --json)")
    ap.add_argument("--names", help="JSON map from class number to name, as the reference's num_to_dog_name_map.json")
    ap.add_argument("--bf16", action="store_true", help="feed the batches as bf16 (bf16 activation storage)")
    args = ap.parse_args()
    if bool(args.json) != bool(args.h5):
        ap.error("--json and --h5 go together")
    require_gpu()
    names = {}
    if args.names:
        with open(args.names) as f:
            names = json.load(f)

    # decoded images a little larger than the network's input, as a decoder would hand them over
    rng = np.random.default_rng(0)
    raw = (args.size * 5) // 4 + 7
    pre = DeviceImagePreprocessor((args.size, args.size), crop_mode="center")

    def batch():
        images = rng.integers(0, 256, size=(args.batch, raw, raw + 11, 3), dtype=np.uint8)
        X = pre.preprocess_batch(images)
        return X.to(torch.bfloat16) if args.bf16 else X

    batches = [batch() for _ in range(args.batches)]
    if args.json:
        net = ResNet18("", load_layers=False)
        net.load_network_from_json_and_h5(args.json, args.h5)
        net.to_gpu()
    else:
        np.random.seed(0)
        net = ResNet18("DogsImageNet225ResNet18DepSep")
        net.to_gpu()
        onehot = torch.zeros((args.batch, 120), device="cuda")
        onehot[:, 0] = 1.0
        net.forward(batches[0], onehot)

    class_idx, scores = net.predict(batches[0], top=args.top)
    class_idx, scores = class_idx.cpu().numpy(), scores.cpu().numpy()
    for n in range(min(args.show, args.batch)):
        print("###########################")
        for i in range(args.top):
            c = int(class_idx[n, i])
            print("image {}".format(n), c, scores[n, i], names.get(str(c), ""))

    classes = net.forward(batches[0][:1], None, test_mode=True)[1].shape[1]
    labels = [rng.integers(0, classes, size=args.batch).tolist() for _ in batches]
    report = net.evaluate(((X, y, None) for X, y in zip(batches, labels)), top=(1, args.top), confusion=True)
    print(report)
    per = report.per_class_accuracy
    seen = ~np.isnan(per)
    print("per-class accuracy over {} classes with images: mean {:.4f}, worst {:.4f}".format(
        int(seen.sum()), float(per[seen].mean()), float(per[seen].min())))


if __name__ == "__main__":
    main()
