"""BASELINE config 5 (bf16 storage): the depthwise-separable stack with bf16 activations
against the fp64 oracle of the same stack, normwise relative error <= 1e-2 (SURVEY.md 8c,
"bf16 (cfg5): normwise <= 1e-2 against the fp32 restatement") on the output and on every
weight / BatchNorm-parameter gradient; plus the kernel-level contracts of the _bf16 twins
(storage rounding: a bf16 depthwise kernel equals its fp32 twin run on the same bf16-representable
inputs, to bf16 rounding of the outputs; the pointwise GEMMs also round their MFMA operands to
bf16).  Config 5 at its own batch size: tests/test_gpu_bf16_fullsize.py."""
import numpy as np
import pytest
import torch

from dorknet_amd._hip import lib, stream_handle, workspace
from tests._convert import layer_to_oracle, rel_err

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def host(t):
    return t.detach().float().cpu().numpy()


def test_cast_round_trip():
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(4099 * 4, device="cuda", generator=g) * 100
    h = torch.empty(x.numel(), dtype=BF16, device="cuda")
    y = torch.empty_like(x)
    st = stream_handle()
    lib.dk_cast_f32_to_bf16(x.data_ptr(), x.numel(), h.data_ptr(), st)
    lib.dk_cast_bf16_to_f32(h.data_ptr(), x.numel(), y.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(h, x.to(BF16))            # round to nearest even, as torch
    assert torch.equal(y, x.to(BF16).float())


@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_and_pointwise_bf16_match_fp32_twins(stride):
    """On bf16-representable inputs the bf16 entries compute exactly the fp32 entries' values
    and round them once on store."""
    rng = np.random.RandomState(3 + stride)
    N, C, H, W, K = 2, 32, 13, 11, 24
    st = stream_handle()
    xh = nhwc(torch.as_tensor(rng.randn(N, C, H, W).astype(np.float32), device="cuda").to(BF16))
    xf = xh.float().contiguous(memory_format=torch.channels_last)
    w = torch.as_tensor(rng.randn(C, 3, 3).astype(np.float32), device="cuda")
    OH, OW = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    yf = nhwc(torch.empty((N, C, OH, OW), device="cuda"))
    yh = nhwc(torch.empty((N, C, OH, OW), device="cuda", dtype=BF16))
    z = (0, 0, 0, 0, 0, 0)
    lib.dk_dwconv_fwd_ex_f32(xf.data_ptr(), N, H, W, C, w.data_ptr(), 3, 3, stride, 1, 0, yf.data_ptr(), OH, OW, *z,
                             st)
    lib.dk_dwconv_fwd_ex_bf16(xh.data_ptr(), N, H, W, C, w.data_ptr(), 3, 3, stride, 1, 0, yh.data_ptr(), OH, OW,
                              *z, st)
    torch.cuda.synchronize()
    assert torch.equal(yh, yf.to(BF16))
    if stride == 1:
        # the pointwise GEMM runs on bf16 MFMA: its operands are rounded to bf16 (x already is),
        # products are exact and accumulate in fp32 -- so it equals the fp32 GEMM on the
        # bf16-rounded weights up to the accumulation order, i.e. within one bf16 rounding of
        # the output (most elements identical)
        wp = torch.as_tensor(rng.randn(K, C).astype(np.float32), device="cuda")
        wr = wp.to(BF16).float()
        pf = nhwc(torch.empty((N, K, H, W), device="cuda"))
        ph = nhwc(torch.empty((N, K, H, W), device="cuda", dtype=BF16))
        lib.dk_pwconv_fwd_ex_f32(xf.data_ptr(), N, H, W, C, wr.data_ptr(), K, 1, 0, pf.data_ptr(), H, W, *z, 0, st)
        lib.dk_pwconv_fwd_ex_bf16(xh.data_ptr(), N, H, W, C, wp.data_ptr(), K, 1, 0, ph.data_ptr(), H, W, *z, st)
        torch.cuda.synchronize()
        ref = pf.to(BF16)
        ulp = (ref.float().abs() * 2.0 ** -7).clamp_min(1e-30)
        assert float(((ph.float() - ref.float()).abs() / ulp).max()) <= 1.0
        assert float((ph != ref).float().mean()) < 0.02


@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_bf16_statistics_rows(stride):
    """The bf16 depthwise forward runs whole output columns per thread (fewer blocks than the fp32
    forward at OH > 14): dk_dwconv_fwd_bf16_stats_rows gives exactly the rows it writes (a row past
    them stays untouched), and the rows sum to the fp64 statistics of the stored bf16 outputs."""
    rng = np.random.RandomState(11 + stride)
    N, C, H, W = 2, 32, 60, 60
    st = stream_handle()
    xh = nhwc(torch.as_tensor(rng.randn(N, C, H, W).astype(np.float32), device="cuda").to(BF16))
    w = torch.as_tensor(rng.randn(C, 3, 3).astype(np.float32), device="cuda")
    OH, OW = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    rows = lib.dk_dwconv_fwd_bf16_stats_rows(N, OH, OW, C, stride)
    assert 0 < rows < lib.dk_dwconv_fwd_stats_rows(N, OH, OW, C, stride)
    part = torch.full((rows + 1, 2, C), float("nan"), dtype=torch.float64, device="cuda")
    yh = nhwc(torch.empty((N, C, OH, OW), device="cuda", dtype=BF16))
    assert lib.dk_dwconv_fwd_ex_bf16(xh.data_ptr(), N, H, W, C, w.data_ptr(), 3, 3, stride, 1, 0, yh.data_ptr(),
                                     OH, OW, 0, 0, 0, 0, 0, part.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(part[rows]).all())
    s = part[:rows].sum(0)
    y = yh.double()
    ref = torch.stack([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))])
    # (a thread's row of outputs is summed in fp32, the rows in fp64: the fp32 forward's rule)
    assert float((s - ref).norm() / ref.norm()) < 1e-6


def _stack(blocks=None, seed=0):
    from examples.mobilenet_stack import BLOCKS, MobileNetStack
    np.random.seed(seed)
    torch.manual_seed(seed)
    net = MobileNetStack("mbs", blocks=BLOCKS if blocks is None else blocks)
    net.to_gpu()
    for l in net.layers:  # non-trivial BN affine parameters
        if "gamma" in (l.learned_params or {}):
            l.learned_params["gamma"].copy_(1.0 + 0.2 * torch.randn_like(l.learned_params["gamma"]))
            l.learned_params["beta"].copy_(0.1 * torch.randn_like(l.learned_params["beta"]))
    return net


def test_every_layer_bf16_vs_oracle():
    """Each layer of the full 16-unit stack on its own: bf16 input (the previous layer's bf16
    output), bf16 output and input gradient, fp32 parameter gradients -- against the fp64
    oracle fed the same bf16 values.  Per layer the only error is storage rounding."""
    net = _stack()
    rng = np.random.RandomState(5)
    x = nhwc(torch.as_tensor(rng.randn(2, 64, 32, 32).astype(np.float32), device="cuda").to(BF16))
    for l in net.layers:
        o = layer_to_oracle(l)
        y = l.forward(x)
        ref = o.forward(host(x).astype(np.float64))
        assert y.dtype == BF16
        assert rel_err(host(y), ref) <= 1e-2, (l.layer_name, rel_err(host(y), ref))
        dy = nhwc(torch.as_tensor(rng.randn(*y.shape).astype(np.float32), device="cuda").to(BF16))
        dx = l.backward(dy)
        torch.cuda.synchronize()
        dref = o.backward(host(dy).astype(np.float64))
        assert dx.dtype == BF16
        assert rel_err(host(dx), dref) <= 1e-2, (l.layer_name, "dx", rel_err(host(dx), dref))
        for k in (l.grads or {}):
            e = rel_err(host(l.grads[k]).reshape(o.grads[k].shape), o.grads[k])
            assert e <= 1e-2, (l.layer_name, k, e)
        x = y


def _bf16(a):
    """Round fp64 values to bf16 (the storage rounding the GPU path applies)."""
    return torch.as_tensor(a).to(torch.bfloat16).to(torch.float64).numpy()


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_mobilenet_stack_bf16_vs_oracle(monkeypatch, fuse):
    """Forward + backward of the first two blocks (4 units, 16 layers) end to end, fused
    (BN on load, producer statistics, BN-backward partials in the dgrads) and unfused.

    Two references: the plain fp64 oracle (output within 2e-2: eight bf16 GEMM layers of operand
    and storage rounding compound to ~1.05e-2 at this depth; each layer alone is within 1e-2,
    test_every_layer_bf16_vs_oracle), and the oracle with the bf16 path's roundings emulated --
    every tensor the GPU path stores in bf16 is rounded to bf16 at the same point (layer outputs,
    input gradients; in the fused path a BatchNorm's output is never stored, its consumer applies
    it on load, so it is not rounded there unless that consumer is a pointwise layer, whose bf16
    MFMA rounds its operands), and the pointwise weights are rounded (bf16 MFMA operands).  Against
    that emulation the output agrees to 1e-2 and every gradient too, except where the
    quantity is ill-conditioned: the first layer's weight gradient, a sum with heavy
    cancellation (the BatchNorm backward removes dy's per-channel mean), which the storage
    rounding alone moves by ~10 % at this tiny batch; there the bound is that sensitivity
    (the same "excess over the arithmetic's own error" idea as the fp32 tests)."""
    monkeypatch.setenv("DORKNET_FUSE", fuse)
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    from dorknet_amd.layers.activations import ReLu
    from examples.mobilenet_stack import BLOCKS
    net = _stack(BLOCKS[:2])
    olayers = [layer_to_oracle(l) for l in net.layers]
    rng = np.random.RandomState(7)
    X = rng.randn(4, 64, 32, 32).astype(np.float32)
    Xh = nhwc(torch.as_tensor(X, device="cuda").to(BF16))
    Xo = Xh.float().cpu().numpy().astype(np.float64)   # the same (bf16-representable) input
    _, Y = net.forward(Xh, None)
    assert Y.dtype == BF16
    dY = rng.randn(*Y.shape).astype(np.float32)
    dYh = nhwc(torch.as_tensor(dY, device="cuda").to(BF16))
    net.backward(dYh)
    torch.cuda.synchronize()
    # plain fp64 oracle
    a = Xo
    for o in olayers:
        a = o.forward(a)
    assert rel_err(host(Y), a) <= 2e-2, rel_err(host(Y), a)
    # rounding emulation
    from dorknet_amd.layers.pointwise_convolution import PointwiseConvLayer
    elayers = [layer_to_oracle(l) for l in net.layers]
    for l, o in zip(net.layers, elayers):
        if isinstance(l, PointwiseConvLayer):
            o.learned_params["weights"] = _bf16(o.learned_params["weights"])  # bf16 MFMA operand
    fused = fuse == "1"
    a = Xo
    for k, (l, o) in enumerate(zip(net.layers, elayers)):
        a = o.forward(a)
        nxt = net.layers[k + 1] if k + 1 < len(net.layers) else None
        bn_out = isinstance(l, BatchNormLayer) or isinstance(l, ReLu)
        deferred = fused and bn_out and nxt is not None and not isinstance(nxt, ReLu)
        if fused and isinstance(l, BatchNormLayer) and isinstance(nxt, ReLu):
            deferred = k + 2 < len(net.layers)
        if not deferred or isinstance(nxt, PointwiseConvLayer):
            a = _bf16(a)
    assert rel_err(host(Y), a) <= 1e-2, rel_err(host(Y), a)
    d = dYh.float().cpu().numpy().astype(np.float64)
    for o in reversed(elayers):
        d = _bf16(o.backward(d))
    d = dYh.float().cpu().numpy().astype(np.float64)
    for o in reversed(olayers):
        d = o.backward(d)
    report = []
    for l, o, e in zip(net.layers, olayers, elayers):
        for k in (l.grads or {}):
            g = host(l.grads[k]).reshape(o.grads[k].shape)
            err = rel_err(g, e.grads[k])                 # GPU vs the rounding emulation
            sens = rel_err(e.grads[k], o.grads[k])       # what the storage rounding alone moves
            report.append((l.layer_name, k, err, sens))
            # within 1e-2 of the emulation, or -- for a quantity the rounding itself moves by
            # more than that (ill-conditioned: heavy cancellation) -- within that movement:
            # the remaining differences are rounding-boundary flips of the same size
            assert err <= max(1e-2, sens), report[-1]
    assert max(r[2] for r in report) > 0


def _bn(C, rng):
    return [torch.as_tensor(v.astype(np.float32), device="cuda") for v in
            (rng.randn(C) * 0.3, rng.rand(C) + 0.5, 1 + 0.3 * rng.randn(C), 0.2 * rng.randn(C))]


def _h(a):
    return nhwc(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda").to(BF16))


@pytest.mark.parametrize("relu", [0, 1])
def test_bf16_bnbwd_fusions_match_unfused(relu):
    """The BatchNorm-backward-on-load fusions of the bf16 path against the unfused sequence
    (dk_bn_bwd_apply_bf16 writing dy, then the dgrad / wgrad on it):
      * pointwise dgrad (dk_pwconv_dgrad_bnbwd_bf16): dy is rounded to bf16 exactly as the apply
        pass stores it, so dy_out is bit-identical and dx agrees to the MFMA accumulation order;
      * depthwise backward (dk_dwconv_bwd_bnbwd_bf16): dy stays fp32 (never stored), so dx, the
        weight gradient and the input BN's partials differ from the unfused path by dy's bf16
        rounding only -- normwise <= 1e-2."""
    rng = np.random.RandomState(11 + relu)
    N, H, W, C, K = 3, 14, 10, 64, 128
    st = stream_handle()
    # pointwise C -> K; its output xo fed a BN(+ReLU) whose output gradient is g
    xo, g = _h(rng.randn(N, K, H, W)), _h(rng.randn(N, K, H, W))
    po = _bn(K, rng)
    k12 = torch.as_tensor(rng.randn(2 * K).astype(np.float32) * 0.1, device="cuda")
    w = torch.as_tensor(rng.randn(K, C).astype(np.float32) * 0.1, device="cuda")
    xin = _h(rng.randn(N, C, H, W))
    pi = _bn(C, rng)
    dy0 = torch.empty_like(g)
    lib.dk_bn_bwd_apply_bf16(xo.data_ptr(), g.data_ptr(), g.numel(), K, *(t.data_ptr() for t in po), relu,
                             k12.data_ptr(), dy0.data_ptr(), st)
    dx0 = torch.empty_like(xin)
    rows0 = lib.dk_pwconv_dgrad_stats_rows(N, H, W, K, C)
    part0 = torch.zeros((rows0, 2, C), dtype=torch.float64, device="cuda")
    lib.dk_pwconv_dgrad_ex_bf16(dy0.data_ptr(), N, H, W, K, w.data_ptr(), C, 1, dx0.data_ptr(), 0, xin.data_ptr(),
                                *(t.data_ptr() for t in pi), 1, part0.data_ptr(), st)
    dy1, dx1 = torch.empty_like(g), torch.empty_like(xin)
    rows1 = lib.dk_pwconv_dgrad_bnbwd_bf16_stats_rows(N, H, W, K, C)
    part1 = torch.zeros((rows1, 2, C), dtype=torch.float64, device="cuda")
    lib.dk_pwconv_dgrad_bnbwd_bf16(g.data_ptr(), xo.data_ptr(), N, H, W, K, *(t.data_ptr() for t in po), relu,
                                   k12.data_ptr(), dy1.data_ptr(), w.data_ptr(), C, dx1.data_ptr(), 0,
                                   xin.data_ptr(), *(t.data_ptr() for t in pi), 1, part1.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(dy0, dy1)
    assert rel_err(host(dx1), host(dx0)) <= 1e-5
    s0, s1 = part0.sum(0), part1.sum(0)
    assert float((s1 - s0).norm() / s0.norm()) < 1e-4

    # depthwise 3x3 stride 1 on C channels, its output x1 fed a BN(+ReLU) with output gradient g1
    x = _h(rng.randn(N, C, H, W))
    x1, g1 = _h(rng.randn(N, C, H, W)), _h(rng.randn(N, C, H, W))
    po = _bn(C, rng)
    k12 = torch.as_tensor(rng.randn(2 * C).astype(np.float32) * 0.1, device="cuda")
    wd = torch.as_tensor(rng.randn(C, 3, 3).astype(np.float32) * 0.3, device="cuda")
    dyd = torch.empty_like(g1)
    lib.dk_bn_bwd_apply_bf16(x1.data_ptr(), g1.data_ptr(), g1.numel(), C, *(t.data_ptr() for t in po), relu,
                             k12.data_ptr(), dyd.data_ptr(), st)
    nbd = lib.dk_dwconv_dgrad_workspace_bytes(C, 3, 3)
    rowsd = lib.dk_dwconv_dgrad_bf16_stats_rows(N, H, W, C, 1)
    pd0 = torch.zeros((rowsd, 2, C), dtype=torch.float64, device="cuda")
    dxd0 = torch.empty_like(x)
    lib.dk_dwconv_dgrad_ex_bf16(dyd.data_ptr(), N, H, W, C, wd.data_ptr(), 3, 3, 1, 1, dxd0.data_ptr(), H, W,
                                workspace.get(nbd), nbd, 0, xin.data_ptr(), *(t.data_ptr() for t in pi), 1,
                                pd0.data_ptr(), st)
    dw0 = torch.empty_like(wd)
    nbw = lib.dk_dwconv_wgrad_workspace_bytes(N, H, W, C, 3, 3)
    lib.dk_dwconv_wgrad_bnx_bf16(dyd.data_ptr(), x.data_ptr(), N, H, W, C, 3, 3, 1, 1, H, W, 0, 0.0, dw0.data_ptr(),
                                 workspace.get(nbw), nbw, 0, 0, 0, 0, 0, st)
    torch.cuda.synchronize()
    rows = lib.dk_dwconv_bwd_bnbwd_stats_rows(N, H, W, C)
    pd1 = torch.zeros((rows, 2, C), dtype=torch.float64, device="cuda")
    dxd1, dw1 = torch.empty_like(x), torch.empty_like(wd)
    nb = lib.dk_dwconv_bwd_bnbwd_workspace_bytes(N, H, W, C, 3, 3)
    # x as the layer input (no input BN on load, no input-BN partials)
    lib.dk_dwconv_bwd_bnbwd_bf16(g1.data_ptr(), x1.data_ptr(), N, H, W, C, *(t.data_ptr() for t in po), relu,
                                 k12.data_ptr(), x.data_ptr(), wd.data_ptr(), 3, 3, 1, 0.0, dw1.data_ptr(),
                                 dxd1.data_ptr(), 0, 0, 0, 0, 0, 0, 0, workspace.get(nb), nb, st)
    torch.cuda.synchronize()
    assert rel_err(host(dxd1), host(dxd0)) <= 1e-2
    assert rel_err(host(dw1), host(dw0)) <= 1e-2
