"""The LeNet-style network of examples/mnist_lenet.py with every ReLu replaced by one of the activations
the reference lacks:

    --activation leaky    LeakyReLu(alpha)   v > 0 ? v : alpha v
    --activation relu6    ReLu6              min(max(v, 0), 6)
    --activation hswish   HardSwish          v min(max(v + 3, 0), 6) / 6
    --activation silu     SiLu               v / (1 + e^-v)

None of them stores a mask: the backward recomputes the derivative from the layer's input.  The data are
the synthetic digits of mnist_lenet.py.

    python examples/mnist_activations.py --activation silu
    python examples/mnist_activations.py --activation leaky --alpha 0.1
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dorknet_amd.layers.activations import HardSwish, LeakyReLu, ReLu, ReLu6, SiLu  # noqa: E402
from examples.mnist_lenet import MNISTLeNet, synthetic_digits  # noqa: E402

ACTIVATIONS = {"leaky": LeakyReLu, "relu6": ReLu6, "hswish": HardSwish, "silu": SiLu}


class MNISTActivationNet(MNISTLeNet):
    def __init__(self, name, load_layers=True, activation="silu", alpha=0.01, **kwargs):
        super().__init__(name, load_layers, **kwargs)
        if not load_layers:
            return
        cls = ACTIVATIONS[activation]
        for i, l in enumerate(self.layers):
            if type(l) is ReLu:
                name_i = l.layer_name.replace("relu", activation)
                self.layers[i] = cls(name_i, alpha=alpha) if cls is LeakyReLu else cls(name_i)


def main():
    import numpy as np
    import torch
    from dorknet_amd._tensor import as_device
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    ap = argparse.ArgumentParser()
    ap.add_argument("--activation", choices=sorted(ACTIVATIONS), default="silu")
    ap.add_argument("--alpha", type=float, default=0.01, help="LeakyReLu's slope below zero")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--images", type=int, default=4096, help="images per epoch")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--every", type=int, default=8, help="print the mean loss every this many steps")
    args = ap.parse_args()
    np.random.seed(0)
    net = MNISTActivationNet("mnist_" + args.activation, activation=args.activation, alpha=args.alpha)
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
    Xt, yt = synthetic_digits(1024, seed=1)
    _, scores = net.forward(as_device(Xt), None, test_mode=True)
    acc = float((scores.argmax(dim=1).cpu() == torch.as_tensor(yt.argmax(axis=1))).float().mean())
    print("held-out accuracy on 1024 fresh images (same prototypes): {:.3f}".format(acc))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
