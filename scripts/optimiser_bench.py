"""update_weights of the optimisers over ResNet-18-depsep's parameter set (104 tensors,
1,336,312 parameters; examples/resnet18_depsep.py): SGDMomentum (dk_sgd_momentum_multi_f32), SGD
(dk_sgd_multi_f32), RMSProp (dk_rmsprop_multi_f32) and Adam (dk_adam_multi_f32), one multi-tensor
launch each, and Adam with max_grad_norm (the two launches of dk_grad_norm_multi_f32 before the
update).  HIP events around --calls back-to-back update_weights() after a warm-up, --repeats times,
the optimisers taking turns within a repeat; per call: the median over the repeats and their
min-max.  Then the same for the C entries alone on the tables update_weights() built (no Python walk
over the tensors): back-to-back update_weights() calls are paced by the host, the entries alone by
the launches; that section has one more row, the l2 term of the forward pass (the two launches of
dk_l2_loss_multi_f32 over the network's l2-regularised weights).  All share the network's parameters
and gradients; the gradients are small, so the weights stay finite.
    python scripts/optimiser_bench.py [--calls 100] [--repeats 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dorknet_amd._hip import lib, stream_handle, workspace  # noqa: E402
from dorknet_amd.optimisers.Adam import Adam  # noqa: E402
from dorknet_amd.optimisers.clip import measure_grad_norm  # noqa: E402
from dorknet_amd.optimisers.RMSProp import RMSProp  # noqa: E402
from dorknet_amd.optimisers.SGD import SGD  # noqa: E402
from dorknet_amd.optimisers.SGDMomentum import SGDMomentum  # noqa: E402
from examples.resnet18_depsep import ResNet18  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    np.random.seed(0)
    net = ResNet18("bench")
    net.to_gpu()
    opts = [("SGDMomentum", SGDMomentum(net, 1e-4, 0.9)), ("SGD", SGD(net, 1e-4)),
            ("RMSProp", RMSProp(net, 1e-6, 0.9)), ("Adam", Adam(net, 1e-6, weight_decay=0.01)),
            ("Adam+clip", Adam(net, 1e-6, weight_decay=0.01, max_grad_norm=1.0))]
    layers = opts[0][1].learnable_layers
    torch.manual_seed(0)
    for l in layers:
        for k, g in l.grads.items():
            g.copy_(1e-3 * torch.randn_like(g))
    ntens = sum(len(l.learned_params) for l in layers)
    nparam = sum(v.numel() for l in layers for v in l.learned_params.values())
    st = stream_handle()

    # the l2 term of a training forward pass (dk_l2_loss_multi_f32 over the network's l2-regularised
    # weights), on the table the network builds for it
    loss = torch.zeros((), dtype=torch.float32, device="cuda")
    l2_out = net._l2_total(net._l2_plan(), loss)
    l2 = net._l2_table
    l2_nb = lib.dk_l2_multi_workspace_bytes(l2.blocks)
    l2_ws = workspace.get(l2_nb)

    def entry_only(opt):  # the C entries on the tables update_weights built: the launches without the Python walk
        if opt is None:
            lib.dk_l2_loss_multi_f32(l2.ptr, l2.ntens, l2.blocks, loss.data_ptr(), l2_out.data_ptr(), l2_ws, l2_nb, st)
        elif getattr(opt, "max_grad_norm", None) is not None:
            out = measure_grad_norm(opt, opt.max_grad_norm, unchanged=True)  # the cached table: no walk either
            opt._launch(opt._dev.ptr, ntens, opt._dev.blocks, st, out.data_ptr() + 4)
        else:
            opt._launch(opt._dev.ptr, ntens, opt._dev.blocks, st)

    for what, call, rows in (("update_weights()", lambda opt: opt.update_weights(), opts),
                             ("the C entries alone", entry_only, opts + [("l2 term", None)])):
        times = {name: [] for name, _ in rows}
        for r in range(a.repeats + 1):  # repeat 0 is the warm-up (and builds the tables)
            for name, opt in rows:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    call(opt)
                e1.record()
                e1.synchronize()
                if r:
                    times[name].append(1e3 * e0.elapsed_time(e1) / a.calls)
        print("{} tensors, {} parameters; us per call of {} over {} back-to-back calls, {} repeats".format(
            ntens, nparam, what, a.calls, a.repeats))
        for name, _ in rows:
            t = sorted(times[name])
            print("  {:12s} median {:7.2f}  min {:7.2f}  max {:7.2f}".format(name, t[len(t) // 2], t[0], t[-1]))


if __name__ == "__main__":
    main()
