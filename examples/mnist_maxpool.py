"""MNISTNet (examples/mnist_convnet.py; reference: examples/MNIST_basic_convnet.py:15-69) with max
pooling: each of the two 4x4 stride-2 convolutions becomes a 3x3 stride-1 convolution + BN + ReLU
followed by MaxPoolLayer(stride=2) (reference: layers/pooling.py:45-77).  The BatchNorm + ReLU in
front of a pool is applied as the pool loads its window (dk_maxpool_fwd_bnx_*), never written.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dorknet_amd.layers.activations import ReLu  # noqa: E402
from dorknet_amd.layers.batch_norm import BatchNormLayer  # noqa: E402
from dorknet_amd.layers.convolution import ConvLayer  # noqa: E402
from dorknet_amd.layers.dense_layer import DenseLayer  # noqa: E402
from dorknet_amd.layers.losses import SoftmaxWithCrossEntropy  # noqa: E402
from dorknet_amd.layers.pooling import GlobalAveragePoolingLayer, MaxPoolLayer  # noqa: E402
from dorknet_amd.network.feed_forward_network import FeedForwardNetwork  # noqa: E402
from dorknet_amd.regularisers.l2 import l2  # noqa: E402

# (filter block, pooled): a pooled convolution stands where MNISTNet has a 4x4 stride-2 one
CONVS = [((32, 1, 3, 3), False), ((32, 32, 3, 3), False), ((64, 32, 3, 3), True), ((64, 64, 3, 3), False),
         ((128, 64, 3, 3), True)]


class MNISTMaxPoolNet(FeedForwardNetwork):
    def __init__(self, name, load_layers=True):
        super().__init__(name)
        if not load_layers:
            return
        pools = 0
        for i, (shape, pooled) in enumerate(CONVS, start=1):
            self.add_layer(ConvLayer("conv_%d" % i, filter_block_shape=shape, with_bias=False, stride=1,
                                     weight_regulariser=l2(0.0001)))
            self.add_layer(BatchNormLayer("bn_%d" % i, incoming_chans=shape[0]))
            self.add_layer(ReLu("relu_%d" % i))
            if pooled:
                pools += 1
                self.add_layer(MaxPoolLayer("pool_%d" % pools, stride=2))
        self.add_layer(GlobalAveragePoolingLayer("global_pool"))
        self.add_layer(DenseLayer("dense_1", incoming_chans=128, output_dim=10, weight_regulariser=l2(0.0005)))
        self.set_loss_layer(SoftmaxWithCrossEntropy("softmax"))
