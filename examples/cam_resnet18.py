"""Class activation maps of the ResNet-18-depsep model on the GPU (reference:
examples/imagenet_dogs_225_resnet_18_depsep_CAM.py): the three best classes of every image of a batch,
their maps and the maps laid over the images, in one call -- ``net.class_activation_maps(X)``
(dorknet_amd/cam.py).  Each overlay is written as a binary PPM, so no image
library is needed.

    python examples/cam_resnet18.py                                   # fresh weights, synthetic batch
    python examples/cam_resnet18.py --json net.json --h5 weights.h5   # a trained checkpoint
    python examples/cam_resnet18.py --bf16                            # bf16 activation storage
    python examples/cam_resnet18.py --reference-features              # features with batch statistics

Without a checkpoint the network makes one training-mode forward pass over the synthetic batch first:
the running statistics that a test-mode forward pass reads exist only after the first batch.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.resnet18_depsep import ResNet18, synthetic_batch  # noqa: E402


def write_ppm(path, bgr):
    """uint8 (H, W, 3) BGR -> a binary PPM (P6 is RGB)."""
    h, w, _ = bgr.shape
    with open(path, "wb") as f:
        f.write("P6\n{} {}\n255\n".format(w, h).encode("ascii"))
        f.write(bgr[:, :, ::-1].tobytes())


def main():
    import numpy as np
    import torch
    from dorknet_amd._hip import require_gpu
    from dorknet_amd._tensor import as_device
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=225)
    ap.add_argument("--top", type=int, default=3)
    ap.add_argument("--json", help="layer structure of a saved network (with --h5)")
    ap.add_argument("--h5", help="weights of a saved network (with --json)")
    ap.add_argument("--bf16", action="store_true", help="feed the batch as bf16 (bf16 activation storage)")
    ap.add_argument("--reference-features", action="store_true",
                    help="take the features with test_mode=False (batch statistics), as the reference's script does")
    ap.add_argument("--out", default="cam_out", help="directory for the PPM files")
    args = ap.parse_args()
    if bool(args.json) != bool(args.h5):
        ap.error("--json and --h5 go together")
    require_gpu()
    X, _, onehot = synthetic_batch(args.batch, size=args.size)
    X, onehot = as_device(X), as_device(onehot)
    if args.bf16:
        X = X.to(torch.bfloat16)
    if args.json:
        net = ResNet18("", load_layers=False)
        net.load_network_from_json_and_h5(args.json, args.h5)
        net.to_gpu()
    else:
        np.random.seed(0)
        net = ResNet18("DogsImageNet225ResNet18DepSep")
        net.to_gpu()
        net.forward(X, onehot)
    class_idx, masks, overlays = net.class_activation_maps(X, top=args.top,
                                                           feature_test_mode=not args.reference_features)
    torch.cuda.synchronize()
    os.makedirs(args.out, exist_ok=True)
    class_idx, overlays = class_idx.cpu().numpy(), overlays.cpu().numpy()
    for n in range(args.batch):
        print("image {}: top classes {}".format(n, class_idx[n].tolist()))
        for k in range(args.top):
            write_ppm(os.path.join(args.out, "image{}_{}_class{}.ppm".format(n, k, class_idx[n, k])), overlays[n, k])
    print("masks {} {}, overlays {} {}: {} PPM files in {}".format(
        tuple(masks.shape), str(masks.dtype).replace("torch.", ""), overlays.shape, overlays.dtype,
        args.batch * args.top, args.out))


if __name__ == "__main__":
    main()
