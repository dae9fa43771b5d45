"""The residual join's bf16 entry points against their fp32 twins and torch fp64:

  * dk_add_bf16 / dk_bn_add_bf16: y bit-identical to widening both operands (dk_cast_bf16_to_f32, exact),
    the _f32 entry, and one rounding (dk_cast_f32_to_bf16); the mask identical to the fp32 entry's;
  * dk_relu_bwd_bn_partial_bf16: dx = where(mask, dy, 0) bit for bit, and the partial-row contract of
    tests/test_gpu_partial_rows.py (rows from dk_bn_partial_blocks, guard rows, the fp64 sums under
    (k + 4) 2^-24 sum|term|, the armed in-launch fold);
  * dk_pwconv_dgrad_ex_bf16 at stride 2: rows from dk_pwconv_dgrad_bf16_stats_rows, the same contract,
    exact zeros (or the residual, bit for bit) off the sampling lattice, the lattice values within the
    project's bf16 bound (1e-2 normwise) of fp64 dy . W with W rounded to bf16, and the
    refusal of partials together with a residual.
"""
import numpy as np
import pytest
import torch

from dorknet_amd._hip import DK_ERR_ARGS, HipError, lib, stream_handle
from tests._partials import (BF16, CL, F32, K_BN_PARTIAL, K_TILED_BWD, NAN, Case, act, bn_params, bwd_ref, check_bwd,
                             nan_act, ptrs, pw_dgrad, untie, vec)
from tests.test_gpu_partial_rows import row_contract

pytestmark = pytest.mark.gpu


def _widen(t):
    out = torch.empty(t.shape, dtype=F32, device="cuda").contiguous(memory_format=CL)
    lib.dk_cast_bf16_to_f32(t.data_ptr(), t.numel(), out.data_ptr(), stream_handle())
    return out


def _round(t):
    out = torch.empty(t.shape, dtype=BF16, device="cuda").contiguous(memory_format=CL)
    lib.dk_cast_f32_to_bf16(t.data_ptr(), t.numel(), out.data_ptr(), stream_handle())
    return out


def _bits(t):
    return t.view(torch.int16)


# ---- dk_add_bf16 / dk_bn_add_bf16 ----
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("bns", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["plain", "bnA", "bnB", "bnAB"])
@pytest.mark.parametrize("C", [4, 12, 64])
def test_bn_add_bf16_is_the_fp32_entry_rounded_once(C, bns, relu, with_mask):
    rng = np.random.RandomState(100 * C + 10 * bns[0] + 5 * bns[1] + relu)
    st = stream_handle()
    shape = (2, C, 6, 6)  # n = 72 C: no multiple of the grid stride; C = 12 has C % 8 == 4
    a, b = act(rng, shape, BF16), act(rng, shape, BF16)
    n = a.numel()
    ta, tb = bn_params(C, rng), bn_params(C, rng)
    pa = ptrs(ta) + (1,) if bns[0] else (0, 0, 0, 0, 0)
    pb = ptrs(tb) + (0,) if bns[1] else (0, 0, 0, 0, 0)
    y16, y32 = nan_act(shape, BF16), nan_act(shape, F32)
    m16 = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    m32 = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    a32, b32 = _widen(a), _widen(b)
    mp16, mp32 = (m16.data_ptr(), m32.data_ptr()) if with_mask else (0, 0)
    assert lib.dk_bn_add_bf16(a.data_ptr(), *pa, b.data_ptr(), *pb, n, C, relu, y16.data_ptr(), mp16, st) == 0
    assert lib.dk_bn_add_f32(a32.data_ptr(), *pa, b32.data_ptr(), *pb, n, C, relu, y32.data_ptr(), mp32, st) == 0
    want = _round(y32)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y16), _bits(want))
    if with_mask and relu:
        assert torch.equal(m16, m32)
        # (for these inputs no positive fp32 sum rounds to zero: the mask is also y > 0 on the stored y)
        assert torch.equal(m16.view(2, 6, 6, C).bool(), (y16.permute(0, 2, 3, 1) > 0))
    else:
        assert bool((m16 == 7).all()), "the mask was written without being asked for"
    if bns == (0, 0):
        # the plain add: dk_add_bf16 against dk_add_f32 in the same way
        z16, z32 = nan_act(shape, BF16), nan_act(shape, F32)
        m16.fill_(7)
        m32.fill_(7)
        assert lib.dk_add_bf16(a.data_ptr(), b.data_ptr(), n, relu, z16.data_ptr(), mp16, st) == 0
        assert lib.dk_add_f32(a32.data_ptr(), b32.data_ptr(), n, relu, z32.data_ptr(), mp32, st) == 0
        wz = _round(z32)
        torch.cuda.synchronize()
        assert torch.equal(_bits(z16), _bits(wz)) and torch.equal(_bits(z16), _bits(y16))
        assert torch.equal(m16, m32)


def test_add_bf16_scalar_tail():
    """n % 4 != 0 (a dense row matrix): the tail elements take the scalar path."""
    rng = np.random.RandomState(5)
    st = stream_handle()
    a = torch.as_tensor(rng.randn(3, 7).astype(np.float32), device="cuda").to(BF16)
    b = torch.as_tensor(rng.randn(3, 7).astype(np.float32), device="cuda").to(BF16)
    y = torch.full((3, 7), NAN, dtype=BF16, device="cuda")
    m = torch.full((21,), 7, dtype=torch.uint8, device="cuda")
    assert lib.dk_add_bf16(a.data_ptr(), b.data_ptr(), 21, 1, y.data_ptr(), m.data_ptr(), st) == 0
    torch.cuda.synchronize()
    v = a.float() + b.float()
    assert torch.equal(_bits(y), _bits(torch.relu(v).to(BF16)))
    assert torch.equal(m.view(3, 7).bool(), v > 0)


# ---- dk_relu_bwd_bn_partial_bf16 ----
def _relu_bwd_case(C):
    N, H, W = 2, 7, 7
    rng = np.random.RandomState(1000 + C)
    st = stream_handle()
    P = N * H * W
    dy = act(rng, (N, C, H, W), BF16)
    mask = torch.as_tensor((rng.rand(N, H, W, C) > 0.4).astype(np.uint8), device="cuda")
    pi = bn_params(C, rng)
    x = untie(act(rng, (N, C, H, W), BF16), pi)
    dx = nan_act((N, C, H, W), BF16)
    rows = lib.dk_bn_partial_blocks(P, C)
    nb = lib.dk_bn_workspace_bytes(P, C)

    def launch(p):
        return lib.dk_relu_bwd_bn_partial_bf16(dy.data_ptr(), mask.data_ptr(), x.data_ptr(), P, C, *ptrs(pi), 1,
                                               dx.data_ptr(), p, nb, st)
    c = Case("bwd", rows, C, P, launch, [dx], lambda: bwd_ref(dx, x, pi, 1))
    c.keep = (dy, mask, pi, x)
    return c


@pytest.mark.parametrize("C", [4, 64])
def test_relu_bwd_bn_partial_bf16(C):
    case = _relu_bwd_case(C)
    part = row_contract(case)
    dy, mask = case.keep[0], case.keep[1]
    dx = case.outs[0]
    want = torch.where(mask.bool().permute(0, 3, 1, 2), dy, torch.zeros_like(dy))
    assert torch.equal(_bits(dx.contiguous(memory_format=CL)), _bits(want.contiguous(memory_format=CL)))
    # k = 1: every term is widened to fp64 on its own (tests/_partials.py K_BN_PARTIAL, batchnorm.hip:386-387)
    s = part[:case.rows].sum(0)
    ref, mag = case.ref()
    ratio = float(((s - ref).abs() / ((K_BN_PARTIAL[0] + 4) * 2.0 ** -24 * mag).clamp_min(1e-300)).max())
    print("relu_bwd_bn_partial_bf16 C={}: rows {} err/bound {:.3g}".format(C, case.rows, ratio))
    assert float(mag.max()) > 0 and ratio < 1.0, ratio
    check_bwd(case.launch, case.rows, C, case.P)


# ---- dk_pwconv_dgrad_ex_bf16, stride 2 ----
SHAPES = [(128, 64, 2, 7, 7),    # M = 98: a partial tile
          (64, 64, 3, 12, 12)]   # M = 432: several tiles


def _strided_case(K, C, N, OH, OW):
    case = pw_dgrad(BF16, K, C, N, OH, OW, 2)
    case.rows = lib.dk_pwconv_dgrad_bf16_stats_rows(N, OH, OW, K, C, 2)
    return case


def _lattice_ref(dy, w):
    """fp64 dy . W with W rounded to bf16 (the MFMA operand): [N][C][OH][OW]."""
    wq = w.to(BF16).double()
    return torch.einsum("nkhw,kc->nchw", dy.double(), wq)


@pytest.mark.parametrize("K,C,N,OH,OW", SHAPES)
def test_strided_dgrad_bf16_rows_values_and_fold(K, C, N, OH, OW):
    case = _strided_case(K, C, N, OH, OW)
    part = row_contract(case)
    dy, w = case.keep[0], case.keep[1]
    dx = case.outs[0]
    lat = torch.zeros((2 * OH, 2 * OW), dtype=torch.bool, device="cuda")
    lat[::2, ::2] = True
    off = dx[:, :, ~lat]
    assert bool((_bits(off.contiguous()) == 0).all()), "an off-lattice element is not +0"
    got, want = dx[:, :, ::2, ::2].double(), _lattice_ref(dy, w)
    err = float((got - want).norm() / want.norm())
    print("strided dgrad K={} C={} M={}: rows {} lattice error {:.3e}".format(K, C, N * OH * OW, case.rows, err))
    assert err <= 1e-2, err
    # k = 1: g and g * x_hat are widened per element (tests/_partials.py K_TILED_BWD, gemm_engine.h:632-633)
    s = part[:case.rows].sum(0)
    ref, mag = case.ref()
    ratio = float(((s - ref).abs() / ((K_TILED_BWD[0] + 4) * 2.0 ** -24 * mag).clamp_min(1e-300)).max())
    print("  partial sums err/bound {:.3g}".format(ratio))
    assert float(mag.max()) > 0 and ratio < 1.0, ratio
    check_bwd(case.launch, case.rows, C, case.P)


@pytest.mark.parametrize("K,C,N,OH,OW", SHAPES)
def test_strided_dgrad_bf16_residual_and_refusal(K, C, N, OH, OW):
    rng = np.random.RandomState(K + C + N)
    st = stream_handle()
    H, W = 2 * OH, 2 * OW
    dy = act(rng, (N, K, OH, OW), BF16)
    w = vec(rng.randn(K, C) * 0.2)
    res = act(rng, (N, C, H, W), BF16)
    dx = nan_act((N, C, H, W), BF16)
    assert lib.dk_pwconv_dgrad_ex_bf16(dy.data_ptr(), N, OH, OW, K, w.data_ptr(), C, 2, dx.data_ptr(), res.data_ptr(),
                                       0, 0, 0, 0, 0, 0, 0, st) == 0
    torch.cuda.synchronize()
    lat = torch.zeros((H, W), dtype=torch.bool, device="cuda")
    lat[::2, ::2] = True
    assert torch.equal(_bits(dx[:, :, ~lat].contiguous()), _bits(res[:, :, ~lat].contiguous()))
    want = _lattice_ref(dy, w) + res[:, :, ::2, ::2].double()
    err = float((dx[:, :, ::2, ::2].double() - want).norm() / want.norm())
    assert err <= 1e-2, err
    # partials together with a residual at stride 2: refused (off-lattice residual terms would need reducing)
    pi = bn_params(C, rng)
    x = act(rng, (N, C, H, W), BF16)
    rows = lib.dk_pwconv_dgrad_bf16_stats_rows(N, OH, OW, K, C, 2)
    part = torch.empty((rows, 2, C), dtype=torch.float64, device="cuda")
    with pytest.raises(HipError, match=str(DK_ERR_ARGS)):
        lib.dk_pwconv_dgrad_ex_bf16(dy.data_ptr(), N, OH, OW, K, w.data_ptr(), C, 2, dx.data_ptr(), res.data_ptr(),
                                    x.data_ptr(), *ptrs(pi), 1, part.data_ptr(), st)
