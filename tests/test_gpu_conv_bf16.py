"""bf16 activation storage for the dense convolution and the pooling head: the kernel contracts of
dk_conv2d_{fwd_ex,dgrad,dgrad_phase,wgrad,wgrad_bnx}_bf16, dk_colsum_bf16 and dk_gap_{fwd,bwd}_bf16,
ConvLayer / GlobalAveragePoolingLayer / DenseLayer at layer level, and MNISTNet end to end.

Kernel contract.  Operands are bf16-representable; the reference is torch fp64 on the CPU fed the
same x / dy and the weights rounded to bf16 (the MFMA rounds that operand).  With BN (+ReLU) on
load the MFMA operand is bn(x) rounded to bf16 as it is staged; the reference takes that operand
from dk_bn_apply_bf16 (the same bn_out arithmetic, rounded once on store -- an entry point with its
own tests), checks it against the fp64 BatchNorm to bf16 rounding, and pads it with zeros AFTER the
BatchNorm.  Bounds, per element, no element excluded (u = 2^-24, n = the reduction length):
  outputs stored in bf16:  |got - ref| <= 2^-8 (|ref| + a) + a,  a = n u (|x| conv |w|)
                           (fp32 accumulation worst case + the one store rounding);
  fp32 weight gradient:    |got - ref| <= u (n sum|dy||x| + 2 |ref|)
                           (fp32 accumulation worst case + the final cast and the l2 fma; the
                           reference includes l2 * w, so the 2^-8 |ref| slack is not needed).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dorknet_amd._hip import lib, stream_handle, workspace
from tests._convert import layer_to_oracle, rel_err

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
U = 2.0 ** -24
ST = 2.0 ** -8


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def host(t):
    return t.detach().float().cpu().numpy()


def d64(t):
    return t.detach().double().cpu()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


#        N  C  Cp  H   W   K   R  S  stride pad
SHAPES = {
    "3x3s1": (2, 8, 8, 13, 11, 24, 3, 3, 1, 1),
    "4x4s2": (2, 8, 8, 13, 11, 24, 4, 4, 2, 1),
    "5x5s2_c3": (3, 3, 4, 9, 9, 8, 5, 5, 2, 2),      # the 4 stored channels are a padded C = 3
    "3x3s1_deep": (2, 72, 72, 7, 7, 136, 3, 3, 1, 1),  # k-tiles cross tap boundaries; > 2 column tiles
    # 162 pixels (ragged for 64- and 128-pixel tiles), one shape per row tile the bf16 rule picks and the
    # other shapes do not reach: short reduction with > 64 columns (64x64x16: this forward, wide_c's dgrads),
    # long reduction with < 128 columns (128x64x32: wide_c's forward with statistics or BN on load), and
    # 128 columns with a long reduction in the dgrads and with statistics (128x128x32, 8 waves)
    "wide_k": (2, 8, 8, 9, 9, 72, 3, 3, 1, 1),
    "wide_c": (2, 72, 72, 9, 9, 8, 3, 3, 1, 1),
    "c128": (2, 128, 128, 9, 9, 128, 3, 3, 1, 1),
}
NAMES = list(SHAPES)


def out_hw(name):
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1


@functools.lru_cache(maxsize=None)
def data(name):
    """Fixed inputs of one shape: x (bf16, Cp channels, the padding channels zero), dy (bf16),
    w / bias (fp32, NOT bf16-representable: the kernels round w), BN vectors of Cp floats."""
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    OH, OW = out_hw(name)
    rng = np.random.RandomState(100 + NAMES.index(name))
    x = np.zeros((N, Cp, H, W), np.float32)
    x[:, :C] = rng.randn(N, C, H, W)
    d = {"x": nhwc(dev(x).to(BF16)), "dy": nhwc(dev(rng.randn(N, K, OH, OW)).to(BF16)),
         "w": dev(rng.randn(K, C, R, S) * 0.3), "bias": dev(rng.randn(K)),
         "bn": [dev(v) for v in (rng.randn(Cp) * 0.3, rng.rand(Cp) + 0.5, 1 + 0.3 * rng.randn(Cp),
                                 0.5 + 0.2 * rng.randn(Cp))]}
    d["w64"] = d["w"].to(BF16).double().cpu()  # the MFMA operand
    return d


@functools.lru_cache(maxsize=None)
def operand(name, bn):
    """The forward / weight-gradient x operand in fp64 (N, C, H, W): x itself (bn None), or
    bn(x) [+ReLU, bn = 1] rounded to bf16 -- dk_bn_apply_bf16's output, checked against fp64."""
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    d = data(name)
    if bn is None:
        return d64(d["x"])[:, :C]
    y = torch.empty_like(d["x"])
    lib.dk_bn_apply_bf16(d["x"].data_ptr(), d["x"].numel(), Cp, *(t.data_ptr() for t in d["bn"]), bn, y.data_ptr(), 0,
                         stream_handle())
    torch.cuda.synchronize()
    m, i, g, b = (d64(t).view(1, Cp, 1, 1) for t in d["bn"])
    ref = g * ((d64(d["x"]) - m) * i) + b
    if bn:
        ref = ref.clamp_min(0)
    got = d64(y)
    # bf16 rounding of an fp32 evaluation (4 operations) of the fp64 value; a ReLU decision may
    # differ only where the value is within that error of zero
    assert bool(((got - ref).abs() <= ST * ref.abs() + 8 * U * (g * ((d64(d["x"]) - m) * i)).abs() + 8 * U * b.abs()).all())
    return got[:, :C]


@functools.lru_cache(maxsize=None)
def reference(name, bn):
    """fp64 forward / input gradient / weight gradient of one shape and their error scales."""
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    d = data(name)
    xo, w, dy = operand(name, bn), d["w64"], d64(d["dy"])
    xv, wv = xo.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xv, wv, None, st, pad)
    y.backward(dy)
    xa, wa = xo.abs().requires_grad_(True), w.abs().requires_grad_(True)
    ya = F.conv2d(xa, wa, None, st, pad)
    ya.backward(dy.abs())
    return {"y": y.detach(), "ya": ya.detach(), "dx": xv.grad, "dxa": xa.grad, "dw": wv.grad, "dwa": wa.grad}


def stored_bound(ref, scale, n):
    a = n * U * scale
    return ST * (ref.abs() + a) + a


def bn_args(d, bn):
    return (0, 0, 0, 0, 0) if bn is None else (*(t.data_ptr() for t in d["bn"]), bn)


def w_krsc(name):
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    out = torch.empty((K, R, S, Cp), device="cuda")
    lib.dk_conv_weight_krsc_f32(data(name)["w"].data_ptr(), K, C, R, S, Cp, out.data_ptr(), stream_handle())
    return out


def run_fwd(name, bn, bias, stats=None):
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    OH, OW = out_hw(name)
    d = data(name)
    wk = w_krsc(name)
    y = nhwc(torch.empty((N, K, OH, OW), dtype=BF16, device="cuda"))
    r = lib.dk_conv2d_fwd_ex_bf16(d["x"].data_ptr(), N, H, W, Cp, wk.data_ptr(), K, R, S, st, pad,
                                  d["bias"].data_ptr() if bias else 0, y.data_ptr(), OH, OW, *bn_args(d, bn),
                                  0 if stats is None else stats.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert r == 0
    return y


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("bn", [None, 0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_forward_contract(name, bn, bias):
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    ref = reference(name, bn)
    y = d64(run_fwd(name, bn, bias))
    want = ref["y"] + (d64(data(name)["bias"]).view(1, K, 1, 1) if bias else 0)
    err, bound = (y - want).abs(), stored_bound(want, ref["ya"], R * S * Cp)
    print(name, bn, bias, "max err / bound", float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())


def test_padding_is_zero_after_the_batchnorm():
    """3x3 pad 1 with beta != 0: the border outputs see zeros, not bn(0) = beta - gamma mean invstd.
    The same data against a reference that normalises the zero padding misses the bound, so a
    loader that did so would fail test_forward_contract too."""
    name = "3x3s1"
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    d = data(name)
    assert float(torch.stack([t.abs().min() for t in d["bn"][3:]]).min()) > 0.05  # every beta != 0
    ref = reference(name, 0)
    y = d64(run_fwd(name, 0, False))
    bound = stored_bound(ref["y"], ref["ya"], R * S * Cp)
    assert bool(((y - ref["y"]).abs() <= bound).all())
    m, i, g, b = (d64(t).view(1, Cp, 1, 1) for t in d["bn"])
    xp = F.pad(d64(d["x"]), (pad, pad, pad, pad))
    wrong = F.conv2d((g * ((xp - m) * i) + b).to(BF16).double(), d["w64"], None, st, 0)
    border = torch.ones_like(y, dtype=torch.bool)
    border[:, :, 1:-1, 1:-1] = False
    assert bool(((y - wrong).abs() > bound)[border].any())


# dk_conv2d_dgrad_bf16 is the stride-1 entry; the phase entry takes every shape (stride 1 included)
@pytest.mark.parametrize("name,entry", [(n, "phase") for n in NAMES] +
                         [(n, "stride1") for n in NAMES if SHAPES[n][8] == 1])
def test_dgrad_contract(name, entry):
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    OH, OW = out_hw(name)
    d = data(name)
    ref = reference(name, None)
    dx = nhwc(torch.full((N, C, H, W), float("nan"), dtype=BF16, device="cuda"))
    sth = stream_handle()
    if entry == "stride1":
        wc = torch.empty((C, R, S, K), device="cuda")
        lib.dk_conv_weight_crsk_f32(d["w"].data_ptr(), K, C, R, S, wc.data_ptr(), sth)
        r = lib.dk_conv2d_dgrad_bf16(d["dy"].data_ptr(), N, OH, OW, K, wc.data_ptr(), C, R, S, pad, dx.data_ptr(), H, W,
                                     sth)
    else:
        nb = lib.dk_conv2d_dgrad_phase_workspace_bytes(K, C, R, S, st)
        r = lib.dk_conv2d_dgrad_phase_bf16(d["dy"].data_ptr(), N, OH, OW, K, K, d["w"].data_ptr(), C, R, S, st, pad,
                                           dx.data_ptr(), H, W, workspace.get(nb), nb, sth)
    torch.cuda.synchronize()
    assert r == 0
    got = d64(dx)
    err, bound = (got - ref["dx"]).abs(), stored_bound(ref["dx"], ref["dxa"], R * S * K)
    print(name, entry, "max err / bound", float((err / bound).max()))
    assert not bool(torch.isnan(got).any())
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("l2", [0.0, 0.01])
@pytest.mark.parametrize("bn", [None, 0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_wgrad_contract(name, bn, l2):
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    OH, OW = out_hw(name)
    d = data(name)
    ref = reference(name, bn)
    dw = torch.full((K, C, R, S), float("nan"), device="cuda")
    nb = lib.dk_conv2d_wgrad_bf16_workspace_bytes(N, OH, OW, K, Cp, R, S)
    assert nb > 0
    head = (d["dy"].data_ptr(), d["x"].data_ptr(), N, H, W, Cp, C, K, R, S, st, pad, OH, OW,
            d["w"].data_ptr() if l2 else 0, l2, dw.data_ptr(), workspace.get(nb), nb)
    if bn is None:
        r = lib.dk_conv2d_wgrad_bf16(*head, stream_handle())
    else:
        r = lib.dk_conv2d_wgrad_bnx_bf16(*head, *bn_args(d, bn), stream_handle())
    torch.cuda.synchronize()
    assert r == 0
    want = ref["dw"] + l2 * d64(d["w"])  # (the l2 term takes the fp32 weights, not the MFMA operand)
    got = d64(dw)
    err, bound = (got - want).abs(), U * (N * OH * OW * ref["dwa"] + 2 * want.abs())
    print(name, bn, l2, "max err / bound", float((err / bound).max()))
    assert not bool(torch.isnan(got).any())
    assert bool((err <= bound).all()), float((err / bound).max())


def test_wgrad_workspace_is_the_bf16_split():
    """A workspace one byte short of the bf16 query is refused (10002), whatever the fp32 query says."""
    name = "3x3s1"
    N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
    OH, OW = out_hw(name)
    d = data(name)
    dw = torch.empty((K, C, R, S), device="cuda")
    nb = lib.dk_conv2d_wgrad_bf16_workspace_bytes(N, OH, OW, K, Cp, R, S)
    from dorknet_amd._hip import HipError
    with pytest.raises(HipError, match="10002"):
        lib.dk_conv2d_wgrad_bf16(d["dy"].data_ptr(), d["x"].data_ptr(), N, H, W, Cp, C, K, R, S, st, pad, OH, OW, 0, 0.0,
                                 dw.data_ptr(), workspace.get(nb), nb - 1, stream_handle())


def test_bad_arguments_are_refused():
    from dorknet_amd._hip import HipError
    x = nhwc(torch.zeros((1, 8, 5, 5), dtype=BF16, device="cuda"))
    y = nhwc(torch.zeros((1, 8, 5, 5), dtype=BF16, device="cuda"))
    w = torch.zeros((8, 3, 3, 8), device="cuda")
    z = (0, 0, 0, 0, 0, 0)
    for C, K, xo in ((6, 8, 0), (8, 6, 0), (8, 8, 2)):  # C % 4, K % 4, x not 8-byte aligned
        with pytest.raises(HipError, match="10001"):
            lib.dk_conv2d_fwd_ex_bf16(x.data_ptr() + xo, 1, 5, 5, C, w.data_ptr(), K, 3, 3, 1, 1, 0, y.data_ptr(), 5, 5,
                                      *z, stream_handle())


@pytest.mark.parametrize("shape", ["3x3s1", "many_tiles", "wide_k", "wide_k+bn", "wide_c", "c128"])
def test_statistics_rows(shape):
    """part has rows + 1 NaN rows: the entry writes exactly dk_conv2d_fwd_bf16_stats_rows() rows, and
    they sum to the statistics of the stored output within one bf16 rounding per element -- either
    statistics rule (fp32 accumulator or stored value; the entry takes the stored value) passes, a
    missing or doubled row does not."""
    name, _, bn = shape.partition("+")  # "+bn": the same forward with the input BatchNorm on load
    if name in SHAPES:
        N, C, Cp, H, W, K, R, S, st, pad = SHAPES[name]
        OH, OW = out_hw(name)
        rows = lib.dk_conv2d_fwd_bf16_stats_rows(N, OH, OW, K, Cp, R, S)
        part = torch.full((rows + 1, 2, K), float("nan"), dtype=torch.float64, device="cuda")
        y = run_fwd(name, 0 if bn else None, True, part)
    else:
        N, C, H, W, K = 4, 8, 40, 40, 24
        rng = np.random.RandomState(7)
        x = nhwc(dev(rng.randn(N, C, H, W)).to(BF16))
        w = dev(rng.randn(K, 3, 3, C) * 0.3)
        rows = lib.dk_conv2d_fwd_bf16_stats_rows(N, H, W, K, C, 3, 3)
        assert rows > 4  # several M tiles
        part = torch.full((rows + 1, 2, K), float("nan"), dtype=torch.float64, device="cuda")
        y = nhwc(torch.empty((N, K, H, W), dtype=BF16, device="cuda"))
        assert lib.dk_conv2d_fwd_ex_bf16(x.data_ptr(), N, H, W, C, w.data_ptr(), K, 3, 3, 1, 1, 0, y.data_ptr(), H, W,
                                         0, 0, 0, 0, 0, part.data_ptr(), stream_handle()) == 0
        torch.cuda.synchronize()
    assert rows > 0
    assert bool(torch.isnan(part[rows]).all())
    assert not bool(torch.isnan(part[:rows]).any())
    s = part[:rows].sum(0).cpu()
    yh = d64(y)
    s1, s1a, s2 = yh.sum((0, 2, 3)), yh.abs().sum((0, 2, 3)), (yh * yh).sum((0, 2, 3))
    print(shape, rows, float(((s[0] - s1).abs() / (ST * s1a)).max()), float(((s[1] - s2).abs() / (2 * ST * s2)).max()))
    assert bool(((s[0] - s1).abs() <= ST * s1a).all())
    assert bool(((s[1] - s2).abs() <= 2 * ST * s2).all())


def test_statistics_take_an_armed_fold():
    """With an in-launch fold armed for exactly the queried rows the forward returns DK_FOLDED and
    finalizes what the separate fold computes from the same rows (tests/_partials.check_stats, the
    check every other partial-row producer gets); unarmed it returns 0."""
    from tests._partials import check_stats
    N, C, H, W, K = 4, 8, 40, 40, 24
    rng = np.random.RandomState(13)
    x = nhwc(dev(rng.randn(N, C, H, W)).to(BF16))
    w = dev(rng.randn(K, 3, 3, C) * 0.3)
    y = nhwc(torch.empty((N, K, H, W), dtype=BF16, device="cuda"))
    rows = lib.dk_conv2d_fwd_bf16_stats_rows(N, H, W, K, C, 3, 3)
    st = stream_handle()

    def launch(p):
        return lib.dk_conv2d_fwd_ex_bf16(x.data_ptr(), N, H, W, C, w.data_ptr(), K, 3, 3, 1, 1, 0, y.data_ptr(), H, W,
                                         0, 0, 0, 0, 0, p, st)
    check_stats(launch, rows, K, N * H * W, rng)


def test_colsum_bf16():
    P, K = 286, 24
    rng = np.random.RandomState(21)
    dy = dev(rng.randn(P, K)).to(BF16)
    out = torch.full((K,), float("nan"), device="cuda")
    nb = lib.dk_colsum_workspace_bytes(P, K)
    assert lib.dk_colsum_bf16(dy.data_ptr(), P, K, out.data_ptr(), workspace.get(nb), nb, stream_handle()) == 0
    torch.cuda.synchronize()
    ref = d64(dy)
    err = (d64(out) - ref.sum(0)).abs()
    assert bool((err <= P * U * ref.abs().sum(0)).all()), float(err.max())


@pytest.mark.parametrize("hw", [(7, 7), (5, 3)])
def test_gap_bf16(hw):
    N, C = 3, 20
    H, W = hw
    rng = np.random.RandomState(31 + H)
    x = nhwc(dev(rng.randn(N, C, H, W)).to(BF16))
    out = torch.full((N, C), float("nan"), device="cuda")
    assert lib.dk_gap_fwd_bf16(x.data_ptr(), N, H * W, C, out.data_ptr(), stream_handle()) == 0
    torch.cuda.synchronize()
    x64 = d64(x)
    err = (d64(out) - x64.mean((2, 3))).abs()
    assert bool((err <= H * W * U * (x64.abs() / (H * W)).sum((2, 3))).all()), float(err.max())
    # backward: fp32 [N, C] gradient -> bf16 dx = the fp32 twin's product (1/HW) * dy, rounded once
    dy = dev(rng.randn(N, C))
    dx = nhwc(torch.full((N, C, H, W), float("nan"), dtype=BF16, device="cuda"))
    dxf = nhwc(torch.empty((N, C, H, W), device="cuda"))
    assert lib.dk_gap_bwd_bf16(dy.data_ptr(), N, H * W, C, dx.data_ptr(), stream_handle()) == 0
    lib.dk_gap_bwd_f32(dy.data_ptr(), N, H * W, C, dxf.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    prod = (dy * torch.tensor(1.0 / (H * W), dtype=torch.float32, device="cuda")).to(BF16)
    assert torch.equal(dx, prod.view(N, C, 1, 1).expand(N, C, H, W))
    assert torch.equal(dx, dxf.to(BF16))
    exact = d64(dy).view(N, C, 1, 1) / (H * W)
    assert bool(((d64(dx) - exact).abs() <= (ST + 4 * U) * exact.abs()).all())


# ---------------------------------------------------------------------------------------
# Layer level
# ---------------------------------------------------------------------------------------

def _conv_layer(shape, stride, padding, bias, seed):
    from dorknet_amd.layers.convolution import ConvLayer
    from dorknet_amd.regularisers.l2 import l2
    np.random.seed(seed)
    l = ConvLayer("conv_t", filter_block_shape=shape, stride=stride, padding=padding, with_bias=bias,
                  weight_regulariser=l2(0.01))
    l.to_gpu()
    if bias:
        l.learned_params["bias"].copy_(torch.randn_like(l.learned_params["bias"]))
    return l


@pytest.mark.parametrize("cfg", [((24, 8, 3, 3), 1, 1, True), ((24, 8, 3, 3), 1, 1, False),
                                 ((24, 8, 4, 4), 2, 1, True), ((24, 8, 4, 4), 2, 1, False),
                                 ((8, 3, 5, 5), 2, 2, True)])
def test_conv_layer_bf16_vs_oracle(cfg):
    """ConvLayer on a bf16 input against the fp64 oracle fed the same values: y, dx and every
    gradient within 1e-2 normwise (the project's bf16 bound); y and dx are bf16.
    The last case has C = 3: the input is channel-padded to 4 and runs the engine path."""
    shape, stride, padding, bias = cfg
    l = _conv_layer(shape, stride, padding, bias, seed=3)
    o = layer_to_oracle(l)
    rng = np.random.RandomState(17)
    x = nhwc(dev(rng.randn(2, shape[1], 13, 11)).to(BF16))
    y = l.forward(x)
    ref = o.forward(host(x).astype(np.float64))
    assert y.dtype == BF16 and l.X.dtype == BF16 and tuple(y.shape) == ref.shape
    assert rel_err(host(y), ref) <= 1e-2, rel_err(host(y), ref)
    dy = nhwc(dev(rng.randn(*y.shape)).to(BF16))
    dx = l.backward(dy)
    torch.cuda.synchronize()
    dref = o.backward(host(dy).astype(np.float64))
    assert dx.dtype == BF16 and tuple(dx.shape) == tuple(x.shape)
    assert rel_err(host(dx), dref) <= 1e-2, rel_err(host(dx), dref)
    assert set(l.grads) == set(o.grads)
    for k in l.grads:
        assert l.grads[k].dtype == torch.float32
        e = rel_err(host(l.grads[k]).reshape(o.grads[k].shape), o.grads[k])
        assert e <= 1e-2, (k, e)


def test_conv_layer_bf16_bn_on_load_and_statistics():
    """A BNOut whose raw input is bf16 is applied on load, and a bn_stats request is served by the
    bf16 row query: the output equals the layer run on the materialised BatchNorm output to the
    accumulation order, and the rows sum to the statistics of the stored output."""
    from dorknet_amd.layers._bn_input import BNOut
    from dorknet_amd.layers._chain import StatsRequest
    l = _conv_layer((24, 8, 3, 3), 1, 1, False, seed=5)
    rng = np.random.RandomState(23)
    x = nhwc(dev(rng.randn(2, 8, 13, 11)).to(BF16))
    bn = [dev(v) for v in (rng.randn(8) * 0.3, rng.rand(8) + 0.5, 1 + 0.3 * rng.randn(8), 0.5 + 0.2 * rng.randn(8))]
    req = StatsRequest()
    y1 = l.forward(BNOut(x, *bn, True), bn_stats=req)
    assert l._bn_in is not None and l.X is x and y1.dtype == BF16
    dy = nhwc(dev(rng.randn(*y1.shape)).to(BF16))
    dx1 = l.backward(dy)
    gw1 = l.grads["weights"].clone()
    y0 = l.forward(BNOut(x, *bn, True).materialize())
    dx0 = l.backward(dy)
    torch.cuda.synchronize()
    assert req.part is not None and req.rows == lib.dk_conv2d_fwd_bf16_stats_rows(2, 13, 11, 24, 8, 3, 3)
    s = req.part.sum(0).cpu()
    yh = d64(y1)
    assert bool(((s[0] - yh.sum((0, 2, 3))).abs() <= 1e-9 * yh.abs().sum((0, 2, 3))).all())
    assert bool(((s[1] - (yh * yh).sum((0, 2, 3))).abs() <= 1e-9 * (yh * yh).sum((0, 2, 3))).all())
    assert rel_err(host(y1), host(y0)) <= 1e-3
    assert torch.equal(dx1, dx0)  # (the dgrad does not read x)
    assert rel_err(host(gw1), host(l.grads["weights"])) <= 1e-5


def test_refusals():
    from dorknet_amd.layers.dense_layer import DenseLayer
    rng = np.random.RandomState(29)
    x = nhwc(dev(rng.randn(2, 8, 9, 9)).to(BF16))
    l10 = _conv_layer((10, 8, 3, 3), 1, 1, False, seed=7)
    with pytest.raises(NotImplementedError, match="conv_t"):
        l10.forward(x)
    l = _conv_layer((24, 8, 3, 3), 1, 1, False, seed=7)
    y = l.forward(x)
    with pytest.raises(NotImplementedError, match="conv_t"):
        l.backward(torch.zeros(tuple(y.shape), device="cuda"))   # an fp32 gradient, bf16 stored input
    l.forward(x.float())
    with pytest.raises(NotImplementedError, match="conv_t"):
        l.backward(torch.zeros_like(y))                           # a bf16 gradient, fp32 stored input
    np.random.seed(1)
    dl = DenseLayer("dense_t", incoming_chans=16, output_dim=4)
    dl.to_gpu()
    with pytest.raises(NotImplementedError, match="dense_t"):
        dl.forward(torch.zeros((2, 16), dtype=BF16, device="cuda"))
    dl.forward(torch.zeros((2, 16), device="cuda"))
    with pytest.raises(NotImplementedError, match="dense_t"):
        dl.backward(torch.zeros((2, 4), dtype=BF16, device="cuda"))


def test_pooling_layer_bf16():
    from dorknet_amd.layers.pooling import GlobalAveragePoolingLayer
    g = GlobalAveragePoolingLayer("gap_t")
    g.to_gpu()
    rng = np.random.RandomState(37)
    x = nhwc(dev(rng.randn(3, 20, 5, 3)).to(BF16))
    y = g.forward(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == (3, 20)
    dx = g.backward(dev(rng.randn(3, 20)))
    assert dx.dtype == BF16 and tuple(dx.shape) == (3, 20, 5, 3)
    yf = g.forward(x.float())
    dxf = g.backward(dev(rng.randn(3, 20)))
    torch.cuda.synchronize()
    assert torch.equal(y, yf) and dxf.dtype == torch.float32  # (bf16 -> fp32 widening is exact)


# ---------------------------------------------------------------------------------------
# Whole network
# ---------------------------------------------------------------------------------------

def _bf16(a):
    """Round fp64 values to bf16 (the storage / MFMA-operand rounding of the GPU path)."""
    return torch.as_tensor(np.ascontiguousarray(a)).to(BF16).to(torch.float64).numpy()


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_mnist_convnet_bf16_vs_oracle(monkeypatch, fuse):
    """MNISTNet (five Conv/BN/ReLU units, GAP, dense, softmax), batch 8, bf16 input: one forward +
    backward, fused and unfused, judged by the method of test_mobilenet_stack_bf16_vs_oracle
    (tests/test_gpu_bf16.py).  Two references: the plain fp64 oracle network (loss within 2e-2,
    the depth-compounding figure that test documents), and the oracle with the GPU path's bf16
    roundings emulated -- conv weights rounded as MFMA operands, every activation below the
    pooling rounded where it is stored or staged (conv outputs; BatchNorm outputs, which are
    stored in bf16 unfused and rounded as the next conv's MFMA operand fused: the same values),
    every input gradient below the pooling rounded as stored.  Every gradient: err <= max(1e-2,
    sens), sens = what the emulated roundings alone move it by.  No gradient is excluded."""
    monkeypatch.setenv("DORKNET_FUSE", fuse)
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    from dorknet_amd.layers.convolution import ConvLayer
    from dorknet_amd.layers.pooling import GlobalAveragePoolingLayer
    from examples.mnist_convnet import MNISTNet
    np.random.seed(0)
    torch.manual_seed(0)
    net = MNISTNet("mnist_bf16")
    net.to_gpu()
    for l in net.layers:  # non-trivial BN affine parameters
        if "gamma" in (l.learned_params or {}):
            l.learned_params["gamma"].copy_(1.0 + 0.2 * torch.randn_like(l.learned_params["gamma"]))
            l.learned_params["beta"].copy_(0.1 * torch.randn_like(l.learned_params["beta"]))
    rng = np.random.RandomState(9)
    Xh = dev(rng.rand(8, 1, 28, 28)).to(BF16)  # 28 x 28 values rounded to bf16
    Xo = Xh.float().cpu().numpy().astype(np.float64)
    onehot = np.eye(10, dtype=np.float32)[rng.randint(0, 10, 8)]
    # every conv output is bf16
    for i in range(1, 6):
        _, a = net.forward(Xh, None, terminal_layer_name="conv_%d" % i)
        assert a.dtype == BF16, i
    loss, P = net.forward(Xh, dev(onehot))
    assert P.dtype == torch.float32
    net.backward()
    torch.cuda.synchronize()
    loss = float(loss)

    def oracle(emulate):
        from oracle.net import ONetwork
        layers = [layer_to_oracle(l) for l in net.layers]
        onet = ONetwork(layers, layer_to_oracle(net.loss_layer))
        if not emulate:
            ol, _ = onet.forward(Xo, onehot.astype(np.float64))
            onet.backward()
            return ol, layers
        below = True  # below the pooling: bf16 storage
        a, reg = Xo, 0.0
        for l, o in zip(net.layers, layers):
            reg += o.regulariser_forward()
            if isinstance(l, ConvLayer):
                w = o.learned_params["weights"]
                o.learned_params["weights"] = _bf16(w)  # bf16 MFMA operand
                a = o.forward(a)
                o.w_plain = w
            else:
                a = o.forward(a)
            if isinstance(l, GlobalAveragePoolingLayer):
                below = False
            if below:
                a = _bf16(a)
        ol, _ = onet.loss_layer.forward(a, onehot.astype(np.float64))
        d = onet.loss_layer.backward()
        for l, o in zip(reversed(net.layers), reversed(layers)):
            if isinstance(l, GlobalAveragePoolingLayer):
                below = True
            d = o.backward(d)
            if below:
                d = _bf16(d)
            if isinstance(l, ConvLayer):
                # the l2 term of the weight gradient takes the fp32 weights, not the MFMA operand
                o.grads["weights"] = o.grads["weights"] + o.l2 * (o.w_plain - o.learned_params["weights"])
        return ol + reg, layers

    oloss, olayers = oracle(False)
    eloss, elayers = oracle(True)
    print("loss", loss, "oracle", oloss, "emulated", eloss)
    assert abs(loss - oloss) <= 2e-2 * abs(oloss), (loss, oloss)
    report = []
    for l, o, e in zip(net.layers, olayers, elayers):
        for k in (l.grads or {}):
            g = host(l.grads[k]).reshape(o.grads[k].shape)
            err = rel_err(g, e.grads[k])             # GPU vs the rounding emulation
            sens = rel_err(e.grads[k], o.grads[k])   # what the roundings alone move it by
            report.append((l.layer_name, k, err, sens))
            print(report[-1])
    for r in report:
        assert r[2] <= max(1e-2, r[3]), r
    assert len(report) == 5 + 2 * 5 + 2 and max(r[2] for r in report) > 0
