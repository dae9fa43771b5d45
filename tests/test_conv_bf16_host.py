"""Host-side checks of the bf16 dense-convolution / pooling-head entry points (no GPU): every
new name is declared in include/dorknet_hip.h, has a perfmodel entry, and the GEMM entries take
the bf16 MFMA peak as their compute roof."""
from dorknet_amd import perfmodel
from dorknet_amd._hip import parse_header

GEMM = ["dk_conv2d_fwd_ex_bf16", "dk_conv2d_dgrad_bf16", "dk_conv2d_dgrad_phase_bf16", "dk_conv2d_wgrad_bf16",
        "dk_conv2d_wgrad_bnx_bf16"]
OTHER = ["dk_colsum_bf16", "dk_gap_fwd_bf16", "dk_gap_bwd_bf16"]
QUERIES = ["dk_conv2d_fwd_bf16_stats_rows", "dk_conv2d_wgrad_bf16_workspace_bytes"]


def test_new_entries_declared_like_their_fp32_twins():
    decls = parse_header()
    for name in GEMM + OTHER + QUERIES:
        assert name in decls, name
    # argument order mirrors the fp32 entry next to it: same argument names, same scalar types;
    # activation pointers are uint16_t (bf16 bits) where the twin's are float
    twins = {"dk_conv2d_fwd_ex_bf16": "dk_conv2d_fwd_ex_f32", "dk_conv2d_dgrad_bf16": "dk_conv2d_dgrad_f32",
             "dk_conv2d_dgrad_phase_bf16": "dk_conv2d_dgrad_phase_f32", "dk_conv2d_wgrad_bf16": "dk_conv2d_wgrad_f32",
             "dk_conv2d_wgrad_bnx_bf16": "dk_conv2d_wgrad_bnx_f32", "dk_colsum_bf16": "dk_colsum_f32",
             "dk_gap_fwd_bf16": "dk_gap_fwd_f32", "dk_gap_bwd_bf16": "dk_gap_bwd_f32",
             "dk_conv2d_fwd_bf16_stats_rows": "dk_conv2d_fwd_stats_rows",
             "dk_conv2d_wgrad_bf16_workspace_bytes": "dk_conv2d_wgrad_workspace_bytes"}
    half = {"x", "y", "dy", "dx", "in"}
    for h, f in twins.items():
        (rh, ph), (rf, pf) = decls[h], decls[f]
        assert rh == rf and [n for _, n in ph] == [n for _, n in pf], (h, f)
        for (th, n), (tf, _) in zip(ph, pf):
            if n in half and "*" in tf and not (h == "dk_gap_bwd_bf16" and n == "dy"):
                assert th == tf.replace("float", "uint16_t"), (h, n, th)
            else:
                assert th == tf, (h, n, th, tf)


def test_new_entries_have_perfmodel_work_and_the_bf16_roof():
    for name in GEMM + OTHER + QUERIES:
        assert name in perfmodel.MODEL, name
    for name in GEMM:
        assert name in perfmodel.BF16_MFMA
        assert perfmodel.peak_tflops(name) == perfmodel.PEAK_BF16_TFLOPS
    for name in OTHER:
        assert perfmodel.peak_tflops(name) == perfmodel.PEAK_F32_TFLOPS
    # BASELINE config 2's convolution (3x3, 64 -> 64 on 256 x 64 x 56 x 56): the fp32 entry's flops, half
    # its bytes, and the roofline bound drops with the roof and the bytes
    N, C, H, K, R = 256, 64, 56, 64, 3
    fwd32 = perfmodel.work("dk_conv2d_fwd_ex_f32", (0, N, H, H, C, 0, K, R, R, 1, 1, 0, 0, H, H, 0, 0, 0, 0, 0, 0, 0))
    fwd16 = perfmodel.work("dk_conv2d_fwd_ex_bf16", (0, N, H, H, C, 0, K, R, R, 1, 1, 0, 0, H, H, 0, 0, 0, 0, 0, 0, 0))
    assert fwd16 == (fwd32[0], fwd32[1] // 2) and fwd16[0] == 2 * N * H * H * K * C * R * R
    dg = perfmodel.work("dk_conv2d_dgrad_bf16", (0, N, H, H, K, 0, C, R, R, 1, 0, H, H, 0))
    ph = perfmodel.work("dk_conv2d_dgrad_phase_bf16", (0, N, H, H, K, K, 0, C, R, R, 1, 1, 0, H, H, 0, 0, 0))
    wg = perfmodel.work("dk_conv2d_wgrad_bf16", (0, 0, N, H, H, C, C, K, R, R, 1, 1, H, H, 0, 0.0, 0, 0, 0, 0))
    wb = perfmodel.work("dk_conv2d_wgrad_bnx_bf16",
                        (0, 0, N, H, H, C, C, K, R, R, 1, 1, H, H, 0, 0.0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    assert dg == ph == wg == wb == fwd16
    assert perfmodel.bound_time_s(*fwd16, "dk_conv2d_fwd_ex_bf16") < perfmodel.bound_time_s(
        *fwd32, "dk_conv2d_fwd_ex_f32")
    assert perfmodel.work("dk_colsum_bf16", (0, 286, 24, 0, 0, 0, 0)) == (286 * 24, 2 * 286 * 24)
    assert perfmodel.work("dk_gap_fwd_bf16", (0, 3, 49, 20, 0, 0))[1] == 2 * (3 * 49 * 20 + 3 * 20)
    assert perfmodel.work("dk_gap_bwd_bf16", (0, 3, 49, 20, 0, 0))[1] == 2 * (3 * 49 * 20 + 3 * 20)
