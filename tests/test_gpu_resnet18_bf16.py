"""ResNet-18-depsep (examples/resnet18_depsep.py) trained end to end with bf16 activation storage: a sanity
test, not parity -- parity is tests/test_gpu_resblock_bf16.py's job (rounding through 34 BatchNorms at
batch 8 is not a meaningful yardstick).  Three SGD-momentum steps on a bf16 batch: every loss, gradient
and updated weight finite, every ResidualBlock output bf16, and the step-0 loss within 2e-2 relative
(the project's bound for a deep bf16 chain, tests/test_gpu_bf16.py) of the fp32 path's on the same
weights and the same bf16-representable input."""
import numpy as np
import pytest
import torch

from tests._convert import all_layers

pytestmark = pytest.mark.gpu


def _net(seed):
    from examples.resnet18_depsep import ResNet18
    np.random.seed(seed)
    net = ResNet18("resnet18_bf16")
    net.to_gpu()
    return net


def test_resnet18_trains_in_bf16(monkeypatch):
    from dorknet_amd.layers.residual_block import ResidualBlock
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    from examples.resnet18_depsep import synthetic_batch
    X, _, onehot = synthetic_batch(8, seed=3)
    Xh = torch.as_tensor(X, device="cuda").to(torch.bfloat16)
    Y = torch.as_tensor(onehot, device="cuda")
    ref = _net(7)
    loss32, _ = ref.forward(Xh.float(), Y)
    loss32 = float(loss32)
    del ref
    net = _net(7)
    block_dtypes = []
    orig = ResidualBlock.forward

    def forward(self, *a, **k):
        out = orig(self, *a, **k)
        block_dtypes.append((self.layer_name, out.dtype))
        return out
    monkeypatch.setattr(ResidualBlock, "forward", forward)
    sgd = SGDMomentum(net, 0.01, 0.9)
    losses = []
    for _ in range(3):
        loss, P = net.forward(Xh, Y)
        net.backward()
        sgd.update_weights()
        losses.append(float(loss))
        assert bool(torch.isfinite(P).all())
        for l in all_layers(net.layers):
            for k, g in (l.grads or {}).items():
                assert bool(torch.isfinite(g).all()), (l.layer_name, k, "gradient")
            for k, w in (l.learned_params or {}).items():
                assert bool(torch.isfinite(w).all()), (l.layer_name, k, "weight")
    print("losses (bf16):", losses, "step-0 loss (fp32):", loss32)
    assert all(np.isfinite(losses))
    assert len(block_dtypes) == 3 * 8 and all(d == torch.bfloat16 for _, d in block_dtypes), block_dtypes
    assert abs(losses[0] - loss32) <= 2e-2 * abs(loss32), (losses[0], loss32)
