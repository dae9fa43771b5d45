"""A LeNet-style network on dorknet_amd: conv -> pool -> flatten -> dense -> dense, the network that
needs ReshapeLayer (reference: layers/reshape.py) to take a pooled 4-D map into a DenseLayer in the
reference's feature order f = c * H * W + h * W + w.

    conv 1->16 + BN + ReLU -> MaxPoolLayer(2)                 28x28 -> 14x14
    conv 16->32 + BN + ReLU -> MaxPoolLayer(2)                14x14 -> 7x7
    conv 32->64 + BN + ReLU -> ReshapeLayer((-1, 64, 7, 7), (-1, 64 * 49))
    DenseLayer 3136 -> 128 -> ReLu -> DenseLayer 128 -> 10 -> softmax

The BatchNorm + ReLU in front of each pool and in front of the reshape is applied as the consumer loads
its input (dk_maxpool_fwd_bnx_*, dk_flatten_fwd_bnx_*), never written.  The data are synthetic MNIST-sized
digits (ten fixed 28x28 prototypes plus noise), so one epoch is learnable and needs no download.

    python examples/mnist_lenet.py                 # one epoch, fp32
    python examples/mnist_lenet.py --bf16          # bf16 activation storage up to the flatten, fp32 head
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dorknet_amd.layers.activations import ReLu  # noqa: E402
from dorknet_amd.layers.batch_norm import BatchNormLayer  # noqa: E402
from dorknet_amd.layers.convolution import ConvLayer  # noqa: E402
from dorknet_amd.layers.dense_layer import DenseLayer  # noqa: E402
from dorknet_amd.layers.losses import SoftmaxWithCrossEntropy  # noqa: E402
from dorknet_amd.layers.pooling import MaxPoolLayer  # noqa: E402
from dorknet_amd.layers.reshape import ReshapeLayer  # noqa: E402
from dorknet_amd.network.feed_forward_network import FeedForwardNetwork  # noqa: E402
from dorknet_amd.regularisers.l2 import l2  # noqa: E402

# (filter block, pooled)
CONVS = [((16, 1, 3, 3), True), ((32, 16, 3, 3), True), ((64, 32, 3, 3), False)]


class MNISTLeNet(FeedForwardNetwork):
    def __init__(self, name, load_layers=True, convs=CONVS, side=28, hidden=128):
        super().__init__(name)
        if not load_layers:
            return
        pools = 0
        for i, (shape, pooled) in enumerate(convs, start=1):
            self.add_layer(ConvLayer("conv_%d" % i, filter_block_shape=shape, with_bias=False, stride=1,
                                     weight_regulariser=l2(0.0001)))
            self.add_layer(BatchNormLayer("bn_%d" % i, incoming_chans=shape[0]))
            self.add_layer(ReLu("relu_%d" % i))
            if pooled:
                pools += 1
                side //= 2
                self.add_layer(MaxPoolLayer("pool_%d" % pools, stride=2))
        C = convs[-1][0][0]
        self.add_layer(ReshapeLayer("flatten", (-1, C, side, side), (-1, C * side * side)))
        self.add_layer(DenseLayer("dense_1", incoming_chans=C * side * side, output_dim=hidden,
                                  weight_regulariser=l2(0.0005)))
        self.add_layer(ReLu("relu_dense_1"))
        self.add_layer(DenseLayer("dense_2", incoming_chans=hidden, output_dim=10, weight_regulariser=l2(0.0005)))
        self.set_loss_layer(SoftmaxWithCrossEntropy("softmax"))


def synthetic_digits(count, seed=0, noise=0.3):
    """`count` 28x28 images in [0, 1]: one of ten fixed smooth prototypes plus noise, and their labels."""
    import numpy as np
    coarse = np.random.default_rng(1234).uniform(0, 1, size=(10, 7, 7)).astype(np.float32)  # the same for every seed
    rng = np.random.default_rng(seed)
    protos = np.kron(coarse, np.ones((4, 4), dtype=np.float32))
    labels = rng.integers(0, 10, count)
    X = protos[labels] + noise * rng.standard_normal((count, 28, 28)).astype(np.float32)
    return np.clip(X, 0, 1)[:, None].astype(np.float32), np.eye(10, dtype=np.float32)[labels]


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
    ap.add_argument("--every", type=int, default=8, help="print the mean loss every this many steps")
    ap.add_argument("--bf16", action="store_true",
                    help="feed the batches as bf16: the convolutions, BatchNorms and pools store bf16 activations, "
                         "the flatten widens them for the fp32 dense head")
    args = ap.parse_args()
    np.random.seed(0)
    net = MNISTLeNet("mnist_lenet")
    net.to_gpu()
    opt = SGDMomentum(net, args.lr, 0.9)
    X, onehot = (as_device(a) for a in synthetic_digits(args.images))
    if args.bf16:
        X = X.to(torch.bfloat16)
    steps = args.images // args.batch
    for epoch in range(args.epochs):
        first = last = None
        window = []
        for i in range(steps):
            s = slice(i * args.batch, (i + 1) * args.batch)
            loss, _ = net.forward(X[s], onehot[s])
            net.backward()
            opt.update_weights()
            window.append(loss)
            if len(window) == args.every or i == steps - 1:
                mean = float(sum(float(v) for v in window) / len(window))
                first = mean if first is None else first
                last = mean
                print("epoch {} step {:3d} mean loss {:.5f}".format(epoch, i, mean))
                window = []
        print("epoch {}: mean loss {:.5f} over the first {} steps, {:.5f} over the last".format(
            epoch, first, args.every, last))
    Xt, yt = synthetic_digits(1024, seed=1)
    Xt = as_device(Xt)
    _, scores = net.forward(Xt.to(torch.bfloat16) if args.bf16 else Xt, None, test_mode=True)
    acc = float((scores.argmax(dim=1).cpu() == torch.as_tensor(yt.argmax(axis=1))).float().mean())
    print("held-out accuracy on 1024 fresh images (same prototypes): {:.3f}".format(acc))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
