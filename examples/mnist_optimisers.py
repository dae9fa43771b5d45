"""The reference's three optimisers (optimisers/SGD.py, optimisers/SGDMomentum.py, optimisers/RMSProp.py)
and, as extensions, Adam (here with decoupled weight decay 0.01 and global-norm clipping at 5) and LARS
(per-tensor trust ratios on the weights, weight decay 1e-4) on
MNISTMaxPoolNet (examples/mnist_maxpool.py) over a fixed synthetic batch: U[0, 1) images with
random labels, which the network memorises.  Prints the loss every few steps and, half way, saves
the optimiser state (save_state_to_h5), builds a new optimiser and restores it (load_state_from_h5),
so the run continues with the velocities / the squared-gradient cache / the moments and step count
it had.

    python examples/mnist_optimisers.py --optimiser rmsprop --steps 40
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.mnist_maxpool import MNISTMaxPoolNet  # noqa: E402


def synthetic_batch(batch, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(batch, 1, 28, 28)).astype(np.float32)
    onehot = np.eye(10, dtype=np.float32)[rng.integers(0, 10, batch)]
    return X, onehot


def make_optimiser(which, net, lr=None):
    from dorknet_amd.optimisers.Adam import Adam
    from dorknet_amd.optimisers.LARS import LARS
    from dorknet_amd.optimisers.RMSProp import RMSProp
    from dorknet_amd.optimisers.SGD import SGD
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    if which == "sgd":
        return SGD(net, 0.05 if lr is None else lr)
    if which == "sgdmomentum":
        return SGDMomentum(net, 0.01 if lr is None else lr, 0.9)
    if which == "adam":
        return Adam(net, 0.001 if lr is None else lr, weight_decay=0.01, max_grad_norm=5.0)
    if which == "lars":
        return LARS(net, 0.02 if lr is None else lr, 0.9, trust_coefficient=0.25, weight_decay=1e-4)
    return RMSProp(net, 0.001 if lr is None else lr, 0.9)


def main():
    import numpy as np
    import torch
    from dorknet_amd._tensor import as_device
    ap = argparse.ArgumentParser()
    ap.add_argument("--optimiser", choices=["sgd", "sgdmomentum", "rmsprop", "adam", "lars"], default="rmsprop")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--every", type=int, default=5, help="print the loss every this many steps")
    args = ap.parse_args()
    np.random.seed(0)
    net = MNISTMaxPoolNet("mnist_maxpool")
    net.to_gpu()
    opt = make_optimiser(args.optimiser, net, args.lr)
    X, onehot = (as_device(a) for a in synthetic_batch(args.batch))
    for i in range(args.steps):
        loss, _ = net.forward(X, onehot)
        net.backward()
        opt.update_weights()
        if i % args.every == 0 or i == args.steps - 1:
            print("step {:3d} loss {:.5f}".format(i, float(loss)))
        if i == args.steps // 2:
            with tempfile.TemporaryDirectory() as d:
                fname = os.path.join(d, "optimiser_state.h5")
                opt.save_state_to_h5(fname)
                opt = make_optimiser(args.optimiser, net, 1.0)  # a fresh one: zero state, another learning rate
                opt.load_state_from_h5(fname)
            print("step {:3d} optimiser state saved and restored into a new {} (learning rate {:g})".format(
                i, type(opt).__name__, opt.learning_rate))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
