"""The fused stride-1 depthwise backward with two output columns per thread
(dk_dwconv_bwd_bnbwd_bf16 / _f32, knob 21 = 2, the default where W >= 12) against the one-column form
(knob 21 = 1): dx bit-identical (same dy values, same tap order), the input BatchNorm's backward
partial sums to fp64 rounding and the weight gradient to fp32 rounding (a thread now sums two
pixels before the block reduction).  The one-column form's parity with the unfused sequence is
test_gpu_bf16.py's; the network's with the oracle test_gpu_bf16_fullsize.py's.
Reference: depthwise_convolution.py:198-221 (backward_cp), batch_norm.py:125-174."""
import numpy as np
import pytest
import torch

from dorknet_amd._hip import lib, stream_handle, workspace

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
COLS_KNOB = 21


def _h(rng, N, C, H, W, dt=BF16):
    a = torch.as_tensor(rng.randn(N, C, H, W).astype(np.float32), device="cuda").to(dt)
    return a.contiguous(memory_format=torch.channels_last)


def _bn(C, rng):
    return [torch.as_tensor(v.astype(np.float32), device="cuda") for v in
            (rng.randn(C) * 0.3, rng.rand(C) + 0.5, 1 + 0.3 * rng.randn(C), 0.2 * rng.randn(C))]


def _run(cols, g, x1, x, wd, po, k12, relu, pi, bn_relu, res, with_dx, with_part):
    N, C, H, W = x.shape
    lib.dk_debug_set_gemm_config(COLS_KNOB, cols)
    bf = x.dtype == BF16
    try:
        rows = (lib.dk_dwconv_bwd_bnbwd_bf16_stats_rows if bf else lib.dk_dwconv_bwd_bnbwd_stats_rows)(N, H, W, C)
        nb = (lib.dk_dwconv_bwd_bnbwd_bf16_workspace_bytes if bf else lib.dk_dwconv_bwd_bnbwd_workspace_bytes)(
            N, H, W, C, 3, 3)
        ws = torch.empty(nb // 4 + 64, dtype=torch.float32, device="cuda")
        part = torch.full((rows, 2, C), float("nan"), dtype=torch.float64, device="cuda") if with_part else None
        dx = torch.full_like(x, float("nan")) if with_dx else None
        dw = torch.full_like(wd, float("nan"))
        bn = (*(t.data_ptr() for t in pi), bn_relu) if pi is not None else (0,) * 5
        rc = (lib.dk_dwconv_bwd_bnbwd_bf16 if bf else lib.dk_dwconv_bwd_bnbwd_f32)(g.data_ptr(), x1.data_ptr(), N, H, W, C, *(t.data_ptr() for t in po), relu,
                                          k12.data_ptr(), x.data_ptr(), wd.data_ptr(), 3, 3, 1, 1e-3, dw.data_ptr(),
                                          dx.data_ptr() if with_dx else 0, res.data_ptr() if res is not None else 0,
                                          *bn, part.data_ptr() if with_part else 0, ws.data_ptr(), nb, stream_handle())
        torch.cuda.synchronize()
    finally:
        lib.dk_debug_set_gemm_config(COLS_KNOB, -1)
    assert rc in (0, 10100), rc
    return rows, dx, dw, part


@pytest.mark.parametrize("N,H,W,C", [(2, 56, 56, 64), (3, 28, 28, 128), (4, 14, 14, 256), (2, 13, 19, 64),
                                     (2, 9, 12, 128), (1, 5, 40, 256)])
@pytest.mark.parametrize("relu,bn_in,stats,resid,with_dx", [(0, True, True, False, True), (1, True, True, True, True),
                                                            (1, True, False, False, True),
                                                            (0, False, False, True, True),
                                                            (1, False, False, False, False)])
@pytest.mark.parametrize("dt", [BF16, torch.float32], ids=["bf16", "f32"])
def test_two_columns_match_one(N, H, W, C, relu, bn_in, stats, resid, with_dx, dt):
    rng = np.random.RandomState(N * 7 + H + W + C + 2 * relu + 3 * bn_in + 5 * resid)
    g, x1, x = _h(rng, N, C, H, W, dt), _h(rng, N, C, H, W, dt), _h(rng, N, C, H, W, dt)
    res = _h(rng, N, C, H, W, dt) if resid else None
    po = _bn(C, rng)
    pi = _bn(C, rng) if bn_in else None
    k12 = torch.as_tensor(rng.randn(2 * C).astype(np.float32) * 0.1, device="cuda")
    wd = torch.as_tensor(rng.randn(C, 3, 3).astype(np.float32) * 0.3, device="cuda")
    args = (g, x1, x, wd, po, k12, relu, pi, 1, res, with_dx, stats)
    rows1, dx1, dw1, p1 = _run(1, *args)
    rows2, dx2, dw2, p2 = _run(2, *args)
    assert rows2 <= rows1  # two columns per thread: at most as many strips
    if with_dx:
        assert torch.equal(dx1, dx2)
    assert bool(torch.isfinite(dw2).all())
    err = float((dw2 - dw1).norm() / dw1.norm())
    assert err < 2e-6, err
    if stats:
        s1, s2 = p1.sum(0), p2.sum(0)
        assert float((s2 - s1).norm() / s1.norm()) < 1e-12


# The smallest shapes that select each block geometry: W < 12 (one column per thread either way),
# a 32-column strip (C / 4 = 16) and a 16-column strip (C / 4 = 32, 14 columns)
SMALL = [(7, 16), (13, 64), (14, 128)]


@pytest.mark.parametrize("W,C", SMALL)
@pytest.mark.parametrize("resid", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("bn_in,stats", [(True, True), (True, False), (False, False)], ids=["part", "bn", "plain"])
@pytest.mark.parametrize("relu", [0, 1], ids=["norelu", "relu"])
@pytest.mark.parametrize("dt", [BF16, torch.float32], ids=["bf16", "f32"])
def test_every_launch_form_at_small_shapes(W, C, relu, bn_in, stats, resid, dt):
    """Every kernel the entry points' launch ladder can pick (storage type x partials / input BN /
    neither x output ReLU x residual x columns per thread), checked as test_two_columns_match_one."""
    test_two_columns_match_one(2, 5, W, C, relu, bn_in, stats, resid, True, dt)


@pytest.mark.parametrize("W,C", SMALL)
@pytest.mark.parametrize("stored_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("resid", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [0, 1], ids=["norelu", "relu"])
@pytest.mark.parametrize("cols", [1, 2])
def test_join_forms_at_small_shapes(W, C, relu, resid, stored_mask, cols):
    """The join entry (dk_dwconv_bwd_bnbwd_join_f32) in every form its launch ladder can pick, against the
    plain entry on the same inputs: dx = (the plain entry's dx, residual included) x (y > 0) bit for bit,
    the weight gradient to fp32 rounding, and the join BatchNorm's partial sums against their fp64
    reference within test_gpu_partial_rows.py's bound."""
    from tests._partials import K_DW_BWD_JOIN, bwd_ref
    N, H = 2, 5
    rng = np.random.RandomState(W + C + 2 * relu + 3 * resid + 5 * stored_mask)
    g, x1 = _h(rng, N, C, H, W, torch.float32), _h(rng, N, C, H, W, torch.float32)
    y = torch.relu(_h(rng, N, C, H, W, torch.float32))
    mask = (y > 0).to(torch.uint8).contiguous(memory_format=torch.channels_last)
    jx = _h(rng, N, C, H, W, torch.float32)
    jp = [torch.as_tensor(v.astype(np.float32), device="cuda") for v in (rng.randn(C) * 0.3, rng.rand(C) + 0.5)]
    res = _h(rng, N, C, H, W, torch.float32) if resid else None
    po = _bn(C, rng)
    k12 = torch.as_tensor(rng.randn(2 * C).astype(np.float32) * 0.1, device="cuda")
    wd = torch.as_tensor(rng.randn(C, 3, 3).astype(np.float32) * 0.3, device="cuda")
    _, dx0, dw0, _ = _run(cols, g, x1, y, wd, po, k12, relu, None, 0, res, True, False)
    lib.dk_debug_set_gemm_config(COLS_KNOB, cols)
    try:
        rows = lib.dk_dwconv_bwd_bnbwd_stats_rows(N, H, W, C)
        nb = lib.dk_dwconv_bwd_bnbwd_workspace_bytes(N, H, W, C, 3, 3)
        ws = torch.empty(nb // 4 + 64, dtype=torch.float32, device="cuda")
        part = torch.full((rows, 2, C), float("nan"), dtype=torch.float64, device="cuda")
        dx, dw = torch.full_like(y, float("nan")), torch.full_like(wd, float("nan"))
        rc = lib.dk_dwconv_bwd_bnbwd_join_f32(g.data_ptr(), x1.data_ptr(), N, H, W, C, *(t.data_ptr() for t in po), relu,
                                              k12.data_ptr(), y.data_ptr(), wd.data_ptr(), 3, 3, 1, 1e-3, dw.data_ptr(),
                                              dx.data_ptr(), res.data_ptr() if resid else 0,
                                              mask.data_ptr() if stored_mask else 0, jx.data_ptr(), jp[0].data_ptr(),
                                              jp[1].data_ptr(), part.data_ptr(), ws.data_ptr(), nb, stream_handle())
        torch.cuda.synchronize()
    finally:
        lib.dk_debug_set_gemm_config(COLS_KNOB, -1)
    assert rc in (0, 10100), rc
    assert torch.equal(dx, dx0 * (y > 0))
    err = float((dw - dw0).norm() / dw0.norm())
    assert err < 2e-6, err
    ref, mag = bwd_ref(dx, jx, jp, 0)
    bound = (K_DW_BWD_JOIN[0] + 4) * 2.0 ** -24 * mag
    assert float(mag.max()) > 0
    assert float(((part.sum(0) - ref).abs() / bound.clamp_min(1e-300)).max()) < 1.0


def test_geometry():
    """Two columns per thread where the width allows (W >= 12, C / 4 a multiple of 16), with the
    strip width that pads the row least; one column otherwise."""
    lib.dk_debug_set_gemm_config(COLS_KNOB, 1)
    try:
        one = {s: lib.dk_dwconv_bwd_bnbwd_bf16_stats_rows(*s) for s in [(64, 56, 56, 64), (64, 14, 14, 256),
                                                                       (64, 7, 7, 512)]}
    finally:
        lib.dk_debug_set_gemm_config(COLS_KNOB, -1)
    assert lib.dk_dwconv_bwd_bnbwd_bf16_stats_rows(64, 7, 7, 512) == one[(64, 7, 7, 512)]
    assert lib.dk_dwconv_bwd_bnbwd_bf16_stats_rows(64, 56, 56, 64) < one[(64, 56, 56, 64)]
    # the fp32 entries (and the join entry) have the same geometry
    assert lib.dk_dwconv_bwd_bnbwd_stats_rows(64, 56, 56, 64) == lib.dk_dwconv_bwd_bnbwd_bf16_stats_rows(64, 56, 56, 64)
