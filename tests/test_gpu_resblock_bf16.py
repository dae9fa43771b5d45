"""ResidualBlock with bf16 activation storage (examples/resnet18_depsep.py's blocks and stem tail) against the
torch fp64 twin with the bf16 path's roundings emulated (tests/_bf16_resblock_twin.py ResBf16Twin).

Bounds (tests/test_gpu_bf16_fullsize.py): the output within 1e-2 normwise of the
emulation and 2e-2 of the plain fp64 twin; every gradient within max(1e-2, sens), sens = emulation vs
plain fp64 (how far the roundings themselves move the quantity).  Every case runs fused and with
DORKNET_FUSE=0, with non-trivial gamma / beta, and also checks

  * every output and input gradient is bf16;
  * the new bf16 entries ran and none of the fp32 join entries ran on activations (dk_add_f32 on a weight
    gradient, add_regulariser_grad, is exempt);
  * a test_mode=True forward is bf16 within 1e-2 of the oracle's test-mode output;
  * the same layers fed fp32 make exactly the entry-point calls recorded on the commit before bf16
    residual storage (FP32_CALLS): fp32 dispatch is untouched.
"""
import numpy as np
import pytest
import torch

from tests._bf16_resblock_twin import ResBf16Twin
from tests._convert import all_layers, layer_to_oracle, rel_err

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
FP32_JOIN = ("dk_add_f32", "dk_bn_add_f32", "dk_relu_bwd_bn_partial_f64")


def _block(name, nf, inc, down):
    """One depthwise-separable residual block of ResNet-18-depsep, as ResNet18.add_res_block builds it."""
    from examples.resnet18_depsep import ResNet18
    net = ResNet18("tmp", load_layers=False)
    net.add_res_block(name, (nf, inc, 3, 3), downsample=down, depthwise_sep=True)
    return net.layers[-1]


def _stem_tail():
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    from dorknet_amd.layers.pointwise_convolution import PointwiseConvLayer
    from dorknet_amd.regularisers.l2 import l2
    return [BatchNormLayer("conv0_bn", input_dimension=4, incoming_chans=64), ReLu("conv0_relu"),
            PointwiseConvLayer("pw0", filter_block_shape=(64, 64), with_bias=False, stride=2,
                               weight_regulariser=l2(0.0001)),
            BatchNormLayer("pw0_bn", input_dimension=4, incoming_chans=64), ReLu("pw0_relu")]


JOIN = {"dk_bn_add_bf16", "dk_relu_bwd_bn_partial_bf16"}
# name -> (layer builder, input shape, seed, new entries the fused run must reach, the same with DORKNET_FUSE=0)
CASES = {
    "identity_res1": (lambda: [_block("res1", 64, 64, False)], (4, 64, 16, 16), 61, JOIN, {"dk_add_bf16"}),
    "downsample_res3": (lambda: [_block("res3", 128, 64, True)], (4, 64, 16, 16), 63,
                        JOIN | {"dk_pwconv_dgrad_ex_bf16"}, {"dk_add_bf16", "dk_pwconv_dgrad_ex_bf16"}),
    "deep_identity_res8": (lambda: [_block("res8", 512, 512, False)], (8, 512, 4, 4), 65, JOIN, {"dk_add_bf16"}),
    "stem_tail": (_stem_tail, (4, 64, 16, 16), 67, {"dk_pwconv_dgrad_ex_bf16", "dk_pwconv_dgrad_bf16_stats_rows"},
                  {"dk_pwconv_dgrad_ex_bf16"}),
    "two_blocks": (lambda: [_block("res2", 64, 64, False), _block("res3", 128, 64, True)], (4, 64, 16, 16), 69,
                   JOIN | {"dk_pwconv_dgrad_ex_bf16"}, {"dk_add_bf16", "dk_pwconv_dgrad_ex_bf16"}),
}

# The entry points each case calls when fed fp32 (forward, backward with the input gradient, a test-mode
# forward), recorded on the commit before this one (bf16 activation storage for ConvLayer and the pooling
# head) with _record below: fp32 inputs must keep taking exactly these.
FP32_CALLS = {
    ("identity_res1", 1): (
        "dk_bn_add_f32 dk_bn_fold_arm_bwd dk_bn_fold_arm_stats dk_bn_infer_params_f32 dk_bn_partial_blocks "
        "dk_bn_partials_workspace_bytes dk_bn_workspace_bytes dk_dwconv_bwd_bnbwd_f32 "
        "dk_dwconv_bwd_bnbwd_stats_rows dk_dwconv_bwd_bnbwd_workspace_bytes dk_dwconv_fwd_ex_f32 "
        "dk_dwconv_fwd_stats_rows dk_l2_loss_f32 dk_pwconv_bwd_bnbwd_f32 dk_pwconv_bwd_fused_preferred "
        "dk_pwconv_bwd_fused_rows dk_pwconv_bwd_fused_workspace_bytes dk_pwconv_fwd_ex_f32 "
        "dk_pwconv_fwd_stats_rows dk_relu_bwd_bn_partial_f64 dk_stream_wait_stream dk_wgrad_reduce_defer "
        "dk_wgrad_reduce_flush dk_wgrad_reduce_pending"
    ).split(),
    ("identity_res1", 0): (
        "dk_add_f32 dk_bn_apply_f32 dk_bn_bwd_f32 dk_bn_bwd_workspace_bytes dk_bn_infer_params_f32 "
        "dk_bn_stats_f32 dk_bn_stats_workspace_bytes dk_dwconv_dgrad_f32 dk_dwconv_dgrad_workspace_bytes "
        "dk_dwconv_fwd_ex_f32 dk_dwconv_wgrad_f32 dk_dwconv_wgrad_workspace_bytes dk_l2_loss_f32 "
        "dk_pwconv_dgrad_f32 dk_pwconv_fwd_f32 dk_pwconv_wgrad_f32 dk_pwconv_wgrad_workspace_bytes "
        "dk_relu_bwd_f32 dk_relu_fwd_f32 dk_stream_wait_stream dk_wgrad_reduce_pending"
    ).split(),
    ("downsample_res3", 1): (
        "dk_bn_add_f32 dk_bn_fold_arm_bwd dk_bn_fold_arm_stats dk_bn_infer_params_f32 dk_bn_partial_blocks "
        "dk_bn_partials_workspace_bytes dk_bn_workspace_bytes dk_dwconv_bwd_bnbwd_f32 "
        "dk_dwconv_bwd_bnbwd_stats_rows dk_dwconv_bwd_bnbwd_workspace_bytes dk_dwconv_bwd_s2_bnbwd_f32 "
        "dk_dwconv_bwd_s2_workspace_bytes dk_dwconv_fwd_ex_f32 dk_dwconv_fwd_stats_rows dk_l2_loss_f32 "
        "dk_pwconv_bwd_bnbwd_f32 dk_pwconv_bwd_fused_preferred dk_pwconv_bwd_fused_rows "
        "dk_pwconv_bwd_fused_workspace_bytes dk_pwconv_dgrad_f32 dk_pwconv_fwd_ex_f32 dk_pwconv_fwd_f32 "
        "dk_pwconv_fwd_stats_rows dk_pwconv_wgrad_f32 dk_pwconv_wgrad_workspace_bytes "
        "dk_relu_bwd_bn_partial_f64 dk_stream_wait_event dk_stream_wait_stream dk_sync_event_record "
        "dk_wgrad_reduce_defer dk_wgrad_reduce_flush dk_wgrad_reduce_pending"
    ).split(),
    ("downsample_res3", 0): (
        "dk_add_f32 dk_bn_apply_f32 dk_bn_bwd_f32 dk_bn_bwd_workspace_bytes dk_bn_infer_params_f32 "
        "dk_bn_stats_f32 dk_bn_stats_workspace_bytes dk_dwconv_dgrad_f32 dk_dwconv_dgrad_workspace_bytes "
        "dk_dwconv_fwd_ex_f32 dk_dwconv_wgrad_f32 dk_dwconv_wgrad_workspace_bytes dk_l2_loss_f32 "
        "dk_pwconv_dgrad_f32 dk_pwconv_fwd_f32 dk_pwconv_wgrad_f32 dk_pwconv_wgrad_workspace_bytes "
        "dk_relu_bwd_f32 dk_relu_fwd_f32 dk_stream_wait_event dk_stream_wait_stream dk_sync_event_record "
        "dk_wgrad_reduce_pending"
    ).split(),
    ("deep_identity_res8", 1): (
        "dk_bn_add_f32 dk_bn_fold_arm_bwd dk_bn_fold_arm_stats dk_bn_infer_params_f32 dk_bn_partial_blocks "
        "dk_bn_partials_workspace_bytes dk_bn_workspace_bytes dk_dwconv_bwd_bnbwd_f32 "
        "dk_dwconv_bwd_bnbwd_stats_rows dk_dwconv_bwd_bnbwd_workspace_bytes dk_dwconv_fwd_ex_f32 "
        "dk_dwconv_fwd_stats_rows dk_l2_loss_f32 dk_pwconv_bwd_fused_rows dk_pwconv_dgrad_bnbwd_f32 "
        "dk_pwconv_dgrad_bnbwd_stats_rows dk_pwconv_fwd_ex_f32 dk_pwconv_fwd_stats_rows "
        "dk_pwconv_wgrad_bnx_f32 dk_pwconv_wgrad_workspace_bytes dk_relu_bwd_bn_partial_f64 "
        "dk_stream_wait_stream dk_wgrad_reduce_defer dk_wgrad_reduce_flush dk_wgrad_reduce_pending"
    ).split(),
    ("deep_identity_res8", 0): (
        "dk_add_f32 dk_bn_apply_f32 dk_bn_bwd_f32 dk_bn_bwd_workspace_bytes dk_bn_infer_params_f32 "
        "dk_bn_stats_f32 dk_bn_stats_workspace_bytes dk_dwconv_dgrad_f32 dk_dwconv_dgrad_workspace_bytes "
        "dk_dwconv_fwd_ex_f32 dk_dwconv_wgrad_f32 dk_dwconv_wgrad_workspace_bytes dk_l2_loss_f32 "
        "dk_pwconv_dgrad_f32 dk_pwconv_fwd_f32 dk_pwconv_wgrad_f32 dk_pwconv_wgrad_workspace_bytes "
        "dk_relu_bwd_f32 dk_relu_fwd_f32 dk_stream_wait_stream dk_wgrad_reduce_pending"
    ).split(),
    ("stem_tail", 1): (
        "dk_bn_apply_f32 dk_bn_bwd_apply_f32 dk_bn_bwd_f32 dk_bn_bwd_workspace_bytes dk_bn_fold_arm_bwd "
        "dk_bn_fold_arm_stats dk_bn_infer_params_f32 dk_bn_partials_workspace_bytes dk_bn_stats_f32 "
        "dk_bn_stats_workspace_bytes dk_l2_loss_f32 dk_pwconv_bwd_fused_rows dk_pwconv_dgrad_ex_f32 "
        "dk_pwconv_dgrad_stats_rows dk_pwconv_fwd_ex_f32 dk_pwconv_fwd_stats_rows dk_pwconv_wgrad_bnx_f32 "
        "dk_pwconv_wgrad_workspace_bytes dk_stream_wait_stream dk_wgrad_reduce_pending"
    ).split(),
    ("stem_tail", 0): (
        "dk_bn_apply_f32 dk_bn_bwd_f32 dk_bn_bwd_workspace_bytes dk_bn_infer_params_f32 dk_bn_stats_f32 "
        "dk_bn_stats_workspace_bytes dk_l2_loss_f32 dk_pwconv_dgrad_f32 dk_pwconv_fwd_f32 dk_pwconv_wgrad_f32 "
        "dk_pwconv_wgrad_workspace_bytes dk_relu_bwd_f32 dk_relu_fwd_f32 dk_stream_wait_stream "
        "dk_wgrad_reduce_pending"
    ).split(),
    ("two_blocks", 1): (
        "dk_bn_add_f32 dk_bn_fold_arm_bwd dk_bn_fold_arm_stats dk_bn_infer_params_f32 dk_bn_partial_blocks "
        "dk_bn_partials_workspace_bytes dk_bn_workspace_bytes dk_dwconv_bwd_bnbwd_f32 "
        "dk_dwconv_bwd_bnbwd_stats_rows dk_dwconv_bwd_bnbwd_workspace_bytes dk_dwconv_bwd_s2_bnbwd_join_f32 "
        "dk_dwconv_bwd_s2_stats_rows dk_dwconv_bwd_s2_workspace_bytes dk_dwconv_dgrad_join_rows "
        "dk_dwconv_fwd_ex_f32 dk_dwconv_fwd_join_f32 dk_dwconv_fwd_stats_rows dk_l2_loss_f32 "
        "dk_pwconv_bwd_bnbwd_f32 dk_pwconv_bwd_fused_preferred dk_pwconv_bwd_fused_rows "
        "dk_pwconv_bwd_fused_workspace_bytes dk_pwconv_dgrad_f32 dk_pwconv_fwd_ex_f32 dk_pwconv_fwd_f32 "
        "dk_pwconv_fwd_stats_rows dk_pwconv_wgrad_f32 dk_pwconv_wgrad_workspace_bytes "
        "dk_relu_bwd_bn_partial_f64 dk_stream_wait_event dk_stream_wait_stream dk_sync_event_record "
        "dk_wgrad_reduce_defer dk_wgrad_reduce_flush dk_wgrad_reduce_pending"
    ).split(),
    ("two_blocks", 0): (
        "dk_add_f32 dk_bn_apply_f32 dk_bn_bwd_f32 dk_bn_bwd_workspace_bytes dk_bn_infer_params_f32 "
        "dk_bn_stats_f32 dk_bn_stats_workspace_bytes dk_dwconv_dgrad_f32 dk_dwconv_dgrad_workspace_bytes "
        "dk_dwconv_fwd_ex_f32 dk_dwconv_wgrad_f32 dk_dwconv_wgrad_workspace_bytes dk_l2_loss_f32 "
        "dk_pwconv_dgrad_f32 dk_pwconv_fwd_f32 dk_pwconv_wgrad_f32 dk_pwconv_wgrad_workspace_bytes "
        "dk_relu_bwd_f32 dk_relu_fwd_f32 dk_stream_wait_event dk_stream_wait_stream dk_sync_event_record "
        "dk_wgrad_reduce_pending"
    ).split(),
}


class _Recorder:
    """Every dk_* entry point called (by name), and for dk_add_f32 the output pointers."""

    def __init__(self, monkeypatch):
        from dorknet_amd import _hip
        self.seen, self.add_out = set(), []
        for n in sorted(_hip.lib.declarations):
            orig = getattr(_hip.lib, n)

            def w(*a, _o=orig, _n=n):
                self.seen.add(_n)
                if _n == "dk_add_f32":
                    self.add_out.append(a[4])
                return _o(*a)
            monkeypatch.setattr(_hip.lib, n, w)


def _build(make, seed):
    np.random.seed(seed)
    layers = make()
    rng = np.random.default_rng(seed + 1)
    for l in all_layers(layers):  # non-trivial BN affine parameters
        if "gamma" in (l.learned_params or {}):
            C = l.incoming_chans
            l.learned_params["gamma"] = (1 + 0.2 * rng.standard_normal((1, C, 1, 1))).astype(np.float32)
            l.learned_params["beta"] = (0.1 * rng.standard_normal((1, C, 1, 1))).astype(np.float32)
    return layers


def _network(layers):
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    net = FeedForwardNetwork("resblock")
    for l in layers:
        net.add_layer(l)
    net.to_gpu()
    return net


def _inputs(shape, seed, dtype):
    X = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(BF16)
    return X, X.to(dtype).to("cuda").contiguous(memory_format=torch.channels_last)


def _step(net, Xd, seed, dtype):
    _, Y = net.forward(Xd, None)
    dY = torch.randn(tuple(Y.shape), generator=torch.Generator().manual_seed(seed + 2)).to(BF16)
    dX = net.backward(dY.to(dtype).to("cuda").contiguous(memory_format=torch.channels_last), input_grad=True)
    _, Yt = net.forward(Xd, None, test_mode=True)
    torch.cuda.synchronize()
    return Y, dY, dX, Yt


def _record(name, fuse, monkeypatch):
    """The fp32 call set of a case (how FP32_CALLS was written)."""
    make, shape, seed, _, _ = CASES[name]
    monkeypatch.setenv("DORKNET_FUSE", "1" if fuse else "0")
    net = _network(_build(make, seed))
    rec = _Recorder(monkeypatch)
    _step(net, _inputs(shape, seed, torch.float32)[1], seed, torch.float32)
    # (dk_sync_event_create runs once per process, at the first cross-stream hand-over: not a case's own call)
    return sorted(rec.seen - {"dk_sync_event_create"})


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", list(CASES))
def test_fp32_calls_unchanged(name, fuse, monkeypatch):
    assert _record(name, fuse, monkeypatch) == sorted(FP32_CALLS[(name, fuse)])


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", list(CASES))
def test_resblock_bf16(name, fuse, monkeypatch):
    make, shape, seed, expect_fused, expect_unfused = CASES[name]
    monkeypatch.setenv("DORKNET_FUSE", "1" if fuse else "0")
    layers = _build(make, seed)
    emu = ResBf16Twin(layers, fuse=bool(fuse))
    plain = ResBf16Twin(layers, emulate=False)
    net = _network(layers)
    rec = _Recorder(monkeypatch)
    X, Xd = _inputs(shape, seed, BF16)
    Y, dY, dX, Yt = _step(net, Xd, seed, BF16)
    assert Y.dtype == BF16 and dX.dtype == BF16 and Yt.dtype == BF16
    expect = expect_fused if fuse else expect_unfused
    assert expect <= rec.seen, sorted(expect - rec.seen)
    grad_ptrs = {g.data_ptr() for l in all_layers(layers) for g in (l.grads or {}).values()}
    assert not [p for p in rec.add_out if p not in grad_ptrs], "dk_add_f32 ran on an activation"
    assert not {"dk_bn_add_f32", "dk_relu_bwd_bn_partial_f64"} & rec.seen, rec.seen & set(FP32_JOIN)
    # test mode against the oracle with the running statistics the training forward left
    h = X.double().numpy()
    for ol in [layer_to_oracle(l) for l in layers]:
        h = ol.forward(h, True)
    e_test = rel_err(Yt.float().cpu().numpy(), h)
    Yg = Y.float().cpu().numpy().astype(np.float64)
    grads = {(l.layer_name, k): l.grads[k].float().cpu().numpy().astype(np.float64)
             for l in all_layers(layers) for k in sorted(l.grads or {})}
    dXg = dX.float().cpu().numpy().astype(np.float64)
    Xn, dYn = X.double().numpy(), dY.double().numpy()
    Ye, dXe, ge = emu.run(Xn, dYn, input_grad=True)
    Yp, dXp, gp = plain.run(Xn, dYn, input_grad=True)
    report = [("Y", rel_err(Yg, Ye), rel_err(Ye, Yp)), ("Y test mode vs oracle", e_test, 0.0),
              ("dX", rel_err(dXg, dXe), rel_err(dXe, dXp))]
    bad = [r for r in report[2:] if r[1] > max(1e-2, r[2])]
    for key, want in ge.items():
        g = grads[key].reshape(want.shape)
        r = (key, rel_err(g, want), rel_err(want, gp[key]))
        report.append(r)
        if r[1] > max(1e-2, r[2]):
            bad.append(r)
    print("case", name, "fused" if fuse else "unfused", "(name, GPU vs emulation, emulation vs plain fp64):")
    for r in report:
        print("  {:40s} {:.3e} {:.3e}".format(str(r[0]), r[1], r[2]))
    assert report[0][1] <= 1e-2, report[0]
    assert rel_err(Yg, Yp) <= 2e-2, ("Y vs plain fp64", rel_err(Yg, Yp))
    assert e_test <= 1e-2, ("test mode", e_test)
    assert not bad, bad
