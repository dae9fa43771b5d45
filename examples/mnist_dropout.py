"""The LeNet-style network of examples/mnist_lenet.py with a DropoutLayer between the two dense layers:

    ... ReshapeLayer -> DenseLayer 3136 -> 128 -> ReLu -> DropoutLayer(0.5) -> DenseLayer 128 -> 10 -> softmax

The mask is a pure function of (seed, step, element index) -- DESIGN.md section 20 -- so the layer stores
no mask, and a run resumed from a checkpoint draws the masks the original run would have drawn.  In test
mode (the held-out accuracy at the end) the layer is the identity.  The data are the synthetic digits of
mnist_lenet.py.

    python examples/mnist_dropout.py                    # one epoch
    python examples/mnist_dropout.py --drop-prob 0.25
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dorknet_amd.layers.dropout import DropoutLayer  # noqa: E402
from examples.mnist_lenet import MNISTLeNet, synthetic_digits  # noqa: E402


class MNISTDropoutNet(MNISTLeNet):
    def __init__(self, name, load_layers=True, drop_prob=0.5, seed=0, **kwargs):
        super().__init__(name, load_layers, **kwargs)
        if not load_layers:
            return
        at = [l.layer_name for l in self.layers].index("dense_2")
        self.layers.insert(at, DropoutLayer("dropout", drop_prob=drop_prob, seed=seed))


def main():
    import numpy as np
    import torch
    from dorknet_amd._tensor import as_device
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--images", type=int, default=4096, help="images per epoch")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--drop-prob", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0, help="the dropout mask's seed")
    ap.add_argument("--every", type=int, default=8, help="print the mean loss every this many steps")
    args = ap.parse_args()
    np.random.seed(0)
    net = MNISTDropoutNet("mnist_dropout", drop_prob=args.drop_prob, seed=args.seed)
    net.to_gpu()
    opt = SGDMomentum(net, args.lr, 0.9)
    X, onehot = (as_device(a) for a in synthetic_digits(args.images))
    steps = args.images // args.batch
    for epoch in range(args.epochs):
        window = []
        for i in range(steps):
            s = slice(i * args.batch, (i + 1) * args.batch)
            loss, _ = net.forward(X[s], onehot[s])
            net.backward()
            opt.update_weights()
            window.append(loss)
            if len(window) == args.every or i == steps - 1:
                print("epoch {} step {:3d} mean loss {:.5f}".format(
                    epoch, i, float(sum(float(v) for v in window) / len(window))))
                window = []
    drop = next(l for l in net.layers if isinstance(l, DropoutLayer))
    print("dropout: {} training forwards, the next mask is that of step {}".format(steps * args.epochs, drop.step))
    Xt, yt = synthetic_digits(1024, seed=1)
    _, scores = net.forward(as_device(Xt), None, test_mode=True)
    acc = float((scores.argmax(dim=1).cpu() == torch.as_tensor(yt.argmax(axis=1))).float().mean())
    print("held-out accuracy on 1024 fresh images (same prototypes): {:.3f}".format(acc))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
