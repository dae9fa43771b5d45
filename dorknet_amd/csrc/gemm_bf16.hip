// bf16 pointwise entry points (BASELINE config 5) and bf16 dense-convolution entry points on the
// implicit-GEMM engine's bf16 MFMA mode (gemm_engine.h).
#include "gemm_engine.h"
#include "pw_launch.h"

using namespace dk;

// ---------------------------------------------------------------------------------------
// bf16 storage twins of the pointwise entries (BASELINE config 5).  Activations bf16,
// weights / statistics / weight gradients fp32; the bodies are the fp32 entries' (gemm_engine.h),
// taking the storage type from their operands.
// ---------------------------------------------------------------------------------------
namespace dk {
// The path of the three bf16 pointwise operations, each read by its row query and its entry: the
// weight-stationary deep kernels (pw_deep_bf16.hip: a side of 256+) before the streaming ones
// (pw_stream_bf16.hip: K, C in {64, 128}; the fused backward K = C = 64) before the tiled engine.
static PwChoice pw16_fwd_choice(int M, int K, int C) {
  return pw_choice(pw_deep16_fwd_plan(M, K, C), pw_stream_bf16_fwd_plan(M, K, C));
}
static PwChoice pw16_dgrad_choice(int M, int K, int C) {
  return pw_choice(pw_deep16_dgrad_plan(M, K, C), pw_stream_bf16_dgrad_plan(M, K, C));
}
static PwChoice pw16_bwd_choice(int M, int K, int C) {
  return pw_choice(pw_deep16_bwd_plan(M, K, C), pw_stream_bf16_bwd_plan(M, K, C));
}
// Launch-only conditions (what the row queries cannot see; DESIGN.md lists them).  A forward or dgrad
// call that fails one of these runs the tiled engine although its shape has a deep or streaming plan:
// with partials, the rows written are then the tiled engine's, not the rows the query reported.
//   * forward: stride 1 on an unpadded grid (dk_pwconv_fwd_bf16_strided_stats_rows is the query that
//     knows the stride), x on a 16-byte boundary (the entry asks for 8), a given input BatchNorm
//     complete and aligned (the tiled engine then refuses the call);
//   * dgrad: g, bn_x and a given dy_out on 16-byte boundaries (the entry asks for 8), and with
//     partials the input BatchNorm complete and aligned (the tiled engine then refuses the call).
static bool pw16_fwd_launch_ok(const bf16_t* x, int stride, int H, int W, int OH, int OW, const float* bn_mean,
                               const float* bn_invstd, const float* bn_gamma, const float* bn_beta) {
  return stride == 1 && H == OH && W == OW && aligned16(x) && (!bn_mean || bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta));
}
static bool pw16_dgrad_launch_ok(const bf16_t* g, const bf16_t* bn_x, const bf16_t* dy_out, const double* part,
                                 const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                 const float* bn_beta) {
  return aligned16(g) && aligned16(bn_x) && (!dy_out || aligned16(dy_out)) &&
         (!part || bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta));
}
}  // namespace dk

// partial-statistics rows of dk_pwconv_fwd_ex_bf16: the deep or streaming plan's, else one per M tile
// of the tiled engine
DK_API int dk_pwconv_fwd_bf16_stats_rows(int N, int OH, int OW, int K, int C) {
  const int M = N * OH * OW;
  const PwChoice c = pw16_fwd_choice(M, K, C);
  return c.path == kPwTiled ? stats_rows(M, K, C, kRowFwdH, kMfBf16) : c.plan.rows;
}
// The same for any stride: the streaming kernels take stride 1 only, a strided launch (the
// N x OH x OW output lattice of a larger input) always runs the tiled engine -- one row per M tile.
DK_API int dk_pwconv_fwd_bf16_strided_stats_rows(int N, int OH, int OW, int K, int C, int stride) {
  if (stride == 1) return dk_pwconv_fwd_bf16_stats_rows(N, OH, OW, K, C);
  return stats_rows(N * OH * OW, K, C, kRowFwdH, kMfBf16);
}

DK_API int dk_pwconv_fwd_ex_bf16(const bf16_t* x, int N, int H, int W, int C, const float* w_kc, int K, int stride,
                                 const float* bias, bf16_t* y, int OH, int OW, const float* bn_mean,
                                 const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                                 double* stats, void* stream) {
  if (C % 4 || K % 4 || !al8(x) || !al8(y) || !aligned16(w_kc) || (bias && !aligned16(bias))) return DK_ERR_ARGS;
  if (!fits((size_t)N * H * W * C * 4) || !fits((size_t)N * OH * OW * K * 4)) return DK_ERR_ARGS;
  const hipStream_t st = as_stream(stream);
  const PwChoice c = pw16_fwd_choice(N * OH * OW, K, C);
  if (c.path != kPwTiled && pw16_fwd_launch_ok(x, stride, H, W, OH, OW, bn_mean, bn_invstd, bn_gamma, bn_beta)) {
    // the deep (pw_deep_bf16.hip) or streaming (pw_stream_bf16.hip) kernel: bit-identical y, its own
    // partial-row grouping
    const int M = N * OH * OW;
    return pw_fold_launch(stats, c.plan, K, [&](const FoldTail* ft) {
      return (c.path == kPwDeep ? pw_deep16_fwd : pw_stream_bf16_fwd)(x, M, w_kc, K, C, bias, y, bn_mean, bn_invstd,
                                                                     bn_gamma, bn_beta, bn_relu, stats, c.plan, st, ft);
    });
  }
  // kRowFwdH: the bf16 pointwise forward's own tile tuning (fp32: kRowPlain), as its row queries above
  return fwd_rows(img1(x, N, H, W, C, OH, OW, stride, N * OH * OW), w_kc, K, C, bias, y, bn_mean, bn_invstd, bn_gamma,
                  bn_beta, bn_relu, stats, kRowFwdH, st);
}

// partial rows of dk_pwconv_dgrad_ex_bf16 (any stride): one per M tile of the tiled engine, the tile
// chosen by the row_config call of the launch below (M x C output, reduction K, plain loaders, bf16 MFMA)
DK_API int dk_pwconv_dgrad_bf16_stats_rows(int N, int OH, int OW, int K, int C, int stride) {
  (void)stride;  // the GEMM is over the N x OH x OW lattice at every stride
  return stats_rows(N * OH * OW, C, K, kRowPlain, kMfBf16);
}

// Pointwise dgrad (bf16): dx = dy . W (+ residual) and, with bn_x/part, the BN-backward partials of
// the BatchNorm whose output the layer consumed.  stride > 1: dx is the widened (OH*stride) x
// (OW*stride) grid, zeros off the sampling lattice (dk_pwconv_dgrad_ex_f32's rules: a residual on
// the widened grid only without part; bn_x on the widened grid).
DK_API int dk_pwconv_dgrad_ex_bf16(const bf16_t* dy, int N, int OH, int OW, int K, const float* w_kc, int C,
                                   int stride, bf16_t* dx, const bf16_t* residual, const bf16_t* bn_x,
                                   const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                   const float* bn_beta, int bn_relu, double* part, void* stream) {
  if (N < 1 || OH < 1 || OW < 1 || K < 4 || C < 4 || stride < 1 || stride > 8) return DK_ERR_ARGS;
  if ((long long)N * OH * OW >= (1ll << 31)) return DK_ERR_ARGS;
  const int M = N * OH * OW;
  if (C % 4 || K % 4 || !dy || !dx || !al8(dy) || !al8(dx) || !aligned16(w_kc)) return DK_ERR_ARGS;
  if ((residual && !al8(residual)) || (bn_x && !al8(bn_x))) return DK_ERR_ARGS;
  if (!fits((size_t)M * K * 4) || !fits((size_t)M * C * 4 * stride * stride) || (part != nullptr) != (bn_x != nullptr))
    return DK_ERR_ARGS;
  if (part && residual && stride != 1) return DK_ERR_ARGS;  // off-lattice residual terms would need reducing
  if (part && !bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta)) return DK_ERR_ARGS;
  return pw_dgrad_tail(dy, M, OH, OW, K, w_kc, C, stride, dx, residual, bn_x,
                       BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, part, as_stream(stream));
}

// dw[k][c] = sum dy[m][k] * bn(x)[m][c] (+ l2 * w), bf16 activations, fp32 result.
DK_API int dk_pwconv_wgrad_bnx_bf16(const bf16_t* dy, const bf16_t* x, int N, int H, int W, int C, int K, int stride,
                                    int OH, int OW, const float* w_kc, float l2, float* dw_kc, void* ws,
                                    size_t ws_bytes, const float* bn_mean, const float* bn_invstd,
                                    const float* bn_gamma, const float* bn_beta, int bn_relu, void* stream) {
  const int Kred = N * OH * OW;
  if (C % 4 || K % 4 || !al8(x) || !al8(dy) || !fits((size_t)N * H * W * C * 4) || !fits((size_t)Kred * K * 4))
    return DK_ERR_ARGS;
  if (ws_bytes < splitk_ws_bytes(K, C, Kred, kMfBf16)) return DK_ERR_WORKSPACE;
  // (the input BatchNorm is looked at after the workspace: callers see this order)
  const ImgDescE<bf16_t> b = img(x, N, H, W, C, OH, OW, 1, 1, stride, 1, 0, Kred);
  if (!bn_mean) return wgrad(dy, b, K, C, w_kc, l2, dw_kc, 0, C, C, 1, 1, ws, ws_bytes, stream);
  if (!bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta)) return DK_ERR_ARGS;
  return wgrad(dy, with_bn(b, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu), K, C, w_kc, l2, dw_kc, 0, C, C, 1, 1, ws,
               ws_bytes, stream);
}

DK_API int dk_pwconv_dgrad_bnbwd_bf16_stats_rows(int N, int OH, int OW, int K, int C) {
  const int M = N * OH * OW;
  const PwChoice c = pw16_dgrad_choice(M, K, C);
  return c.path == kPwTiled ? stats_rows(M, C, K, kRowBnBwd, kMfBf16) : c.plan.rows;
}

// dk_pwconv_dgrad_bnbwd_f32 for bf16 storage: dy = the following BatchNorm's backward applied
// to (g, bn_x) as they are loaded (fp32), rounded to bf16 as the MFMA operand and as stored to
// dy_out (nullable) for the weight gradient; dx = dy . W (+ residual) stored bf16 with, given
// x / part, the input BatchNorm's backward partials over the stored dx.  Stride 1.
DK_API int dk_pwconv_dgrad_bnbwd_bf16(const bf16_t* g, const bf16_t* bn_x, int N, int OH, int OW, int K,
                                      const float* out_mean, const float* out_invstd, const float* out_gamma,
                                      const float* out_beta, int out_relu, const float* k12, bf16_t* dy_out,
                                      const float* w_kc, int C, bf16_t* dx, const bf16_t* residual, const bf16_t* x,
                                      const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                      const float* bn_beta, int bn_relu, double* part, void* stream) {
  const int M = N * OH * OW;
  if (C % 4 || K % 4 || !al8(g) || !al8(bn_x) || !al8(dx) || (dy_out && !al8(dy_out)) || !aligned16(w_kc))
    return DK_ERR_ARGS;
  if ((residual && !al8(residual)) || (x && !al8(x))) return DK_ERR_ARGS;
  if (!fits((size_t)M * K * 4) || !fits((size_t)M * C * 4) || (part != nullptr) != (x != nullptr)) return DK_ERR_ARGS;
  if (!out_mean || !out_invstd || !out_gamma || !out_beta || !k12 || (size_t)K * 32 > 64 * 1024) return DK_ERR_ARGS;
  const PwChoice c = pw16_dgrad_choice(M, K, C);
  if (c.path != kPwTiled && pw16_dgrad_launch_ok(g, bn_x, dy_out, part, bn_mean, bn_invstd, bn_gamma, bn_beta)) {
    // the deep (pw_deep_bf16.hip) or streaming (pw_stream_bf16.hip) kernel: bit-identical dy and dx, its
    // own partial rows
    return pw_fold_launch(part, c.plan, C, [&](const FoldTail* ft) {
      return (c.path == kPwDeep ? pw_deep16_dgrad_bnbwd : pw_stream_bf16_dgrad_bnbwd)(
          g, bn_x, M, K, C, out_mean, out_invstd, out_gamma, out_beta, out_relu, k12, dy_out, w_kc, dx, residual, x,
          bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu, part, c.plan, as_stream(stream), ft);
    });
  }
  if (part && !bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta)) return DK_ERR_ARGS;
  return pw_dgrad_bnbwd_tail(
      with_bnbwd(mat(g, M, K, M), bn_x, BnBwdIn{out_mean, out_invstd, out_gamma, out_beta, k12, out_relu, K}, dy_out), M, K,
      w_kc, C, dx, residual, x, BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, part, as_stream(stream));
}

// Fused pointwise backward for bf16 storage (dk_pwconv_bwd_bnbwd_f32's bf16 twin): the dgrad of
// dk_pwconv_dgrad_bnbwd_bf16 (dy formed on load from (g, bn_x), rounded to bf16 as the MFMA operand,
// dx bit-identical) and the weight gradient dW = dy^T bn_relu(x) (+ l2 w) in one pass, dy never
// stored.  K = C = 64, stride 1 (pw_stream_bf16.hip bwd_fused_kernel); rows = partial rows of part,
// the workspace holds rows fp32 [K][C] weight-gradient partial rows.
DK_API int dk_pwconv_bwd_fused_bf16_rows(int N, int OH, int OW, int K, int C) {
  if (N < 1 || OH < 1 || OW < 1 || (long long)N * OH * OW >= (1ll << 31)) return 0;
  return pw16_bwd_choice(N * OH * OW, K, C).plan.rows;  // (no tiled form: 0)
}

DK_API size_t dk_pwconv_bwd_fused_bf16_workspace_bytes(int N, int OH, int OW, int K, int C) {
  return (size_t)dk_pwconv_bwd_fused_bf16_rows(N, OH, OW, K, C) * K * C * sizeof(float);
}

DK_API int dk_pwconv_bwd_bnbwd_bf16(const bf16_t* g, const bf16_t* bn_x, int N, int OH, int OW, int K,
                                    const float* out_mean, const float* out_invstd, const float* out_gamma,
                                    const float* out_beta, int out_relu, const float* k12, const float* w_kc, int C,
                                    float l2, float* dw_kc, bf16_t* dx, const bf16_t* residual, const bf16_t* x,
                                    const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                    const float* bn_beta, int bn_relu, double* part, void* ws, size_t ws_bytes,
                                    void* stream) {
  const hipStream_t st = as_stream(stream);
  if (N < 1 || OH < 1 || OW < 1 || (long long)N * OH * OW >= (1ll << 31)) return DK_ERR_ARGS;
  const int M = N * OH * OW;
  const PwChoice c = pw16_bwd_choice(M, K, C);
  if (c.path == kPwTiled) return DK_ERR_ARGS;
  if (!g || !bn_x || !x || !w_kc || !dw_kc || !dx || !out_mean || !out_invstd || !out_gamma || !out_beta || !k12)
    return DK_ERR_ARGS;
  if (part && !bn_mean) return DK_ERR_ARGS;
  if (bn_mean && !bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta)) return DK_ERR_ARGS;
  if (!aligned16(g) || !aligned16(bn_x) || !aligned16(w_kc) || !aligned16(ws) || !al8(x) || !al8(dx) ||
      (residual && !al8(residual)))
    return DK_ERR_ARGS;
  if (ws_bytes < (size_t)c.plan.rows * K * C * sizeof(float)) return DK_ERR_WORKSPACE;
  float* wp = static_cast<float*>(ws);
  // K in {128, 256}: the weight-stationary kernel (pw_deep_bf16.hip); it needs the input BN's partials
  // whenever there is an input BN
  if (c.path == kPwDeep && (bn_mean != nullptr) != (part != nullptr)) return DK_ERR_ARGS;
  return pw_bwd_fold_launch(part, c.plan, K, C, wp, w_kc, l2, dw_kc, st, [&](const FoldTail* ft) {
    if (c.path == kPwDeep)
      return pw_deep16_bwd_fused(g, bn_x, M, K, C, out_mean, out_invstd, out_gamma, out_beta, out_relu, k12, w_kc, dx,
                                 residual, x, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu, part, wp, c.plan, st, ft);
    return pw_stream_bf16_bwd_fused(g, bn_x, M, out_mean, out_invstd, out_gamma, out_beta, out_relu, k12, w_kc, dx,
                                    residual, x, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu, part, wp, c.plan, st,
                                    ft);
  });
}

// ---------------------------------------------------------------------------------------
// bf16 storage twins of the dense convolution (layers/convolution.py; gemm_conv.hip holds the fp32
// entries).  x / y / dy / dx bf16 NHWC; weights, bias, BN vectors, statistics and weight gradients
// fp32; every GEMM runs on v_mfma_f32_32x32x16_bf16 (MF = kMfBf16: both operands rounded to bf16 as
// they are staged, products exact, fp32 accumulation).
//
// Loads: a bf16 bload4e moves 8 bytes = 4 channels.  The reduction index k = (tap, c) advances in
// steps of 4 and C % 4 == 0, so a 4-group never straddles a tap; a k-tile may, and each 4-group takes
// its own tap's bounds test (LdImgKC::load), so padding is exactly 0 -- also under BN on load, which
// transforms in-image elements only (ImgBnDescE).
//
// Statistics: taken over the bf16-rounded stored value (EpStoreStatsT<bf16_t>::value4 rounds before
// it accumulates) -- the rule of dk_pwconv_fwd_ex_bf16 and of every other bf16 producer, so that the
// following BatchNorm normalises exactly the tensor its consumers read.
// ---------------------------------------------------------------------------------------

// partial-statistics rows of dk_conv2d_fwd_ex_bf16: one per M tile of the tiled engine
DK_API int dk_conv2d_fwd_bf16_stats_rows(int N, int OH, int OW, int K, int C, int R, int S) {
  return stats_rows(N * OH * OW, K, R * S * C, kRowConv, kMfBf16);
}

DK_API int dk_conv2d_fwd_ex_bf16(const bf16_t* x, int N, int H, int W, int C, const float* w_krsc, int K, int R, int S,
                                 int stride, int pad, const float* bias, bf16_t* y, int OH, int OW,
                                 const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                 const float* bn_beta, int bn_relu, double* stats, void* stream) {
  if (C < 4 || C % 4 || K < 4 || K % 4 || !al8(x) || !al8(y) || !aligned16(w_krsc) || (bias && !aligned16(bias)))
    return DK_ERR_ARGS;
  if (N < 1 || R < 1 || S < 1 || stride < 1 || OH < 1 || OW < 1) return DK_ERR_ARGS;
  if (!fits((size_t)N * H * W * C * 4) || !fits((size_t)N * OH * OW * K * 4)) return DK_ERR_ARGS;
  return fwd_rows(img(x, N, H, W, C, OH, OW, R, S, stride, 1, -pad, N * OH * OW), w_krsc, K, R * S * C, bias, y,
                  bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu, stats, kRowConv, as_stream(stream));
}

// Stride-1 dgrad (dk_conv2d_dgrad_f32's view): dx[n,h,w,c] = sum_{r,s,k} dy[n, h+pad-r, w+pad-s, k] * w[k][c][r][s]
DK_API int dk_conv2d_dgrad_bf16(const bf16_t* dy, int N, int OH, int OW, int K, const float* w_crsk, int C, int R,
                                int S, int pad, bf16_t* dx, int H, int W, void* stream) {
  if (K < 4 || K % 4 || C < 1 || N < 1 || R < 1 || S < 1 || !al8(dy) || !aligned16(w_crsk) || !dx) return DK_ERR_ARGS;
  if (!fits((size_t)N * OH * OW * K * 4) || !fits((size_t)N * H * W * C * 4)) return DK_ERR_ARGS;
  // kRowConv: the bf16 dense dgrads pick their tile as a convolution (the fp32 twins as kRowPlain)
  return dgrad_rows(dy, N, OH, OW, K, w_crsk, C, R, S, pad, dx, H, W, kRowConv, as_stream(stream));
}

// Any-stride dgrad, one implicit GEMM per sub-pixel phase (dk_conv2d_dgrad_phase_f32's geometry and
// workspace: the fp32 phase sub-filters of w_phase_kernel); dy has Kp = K rounded up to 4 channels.
DK_API int dk_conv2d_dgrad_phase_bf16(const bf16_t* dy, int N, int OH, int OW, int Kp, int K, const float* w_kcrs,
                                      int C, int R, int S, int stride, int pad, bf16_t* dx, int H, int W, void* ws,
                                      size_t ws_bytes, void* stream) {
  if (Kp % 4 || Kp < K || K < 1 || stride < 1 || stride > 8 || N < 1 || C < 1 || R < 1 || S < 1 || !al8(dy) || !dx ||
      !aligned16(ws))
    return DK_ERR_ARGS;
  // kRowConv: as dk_conv2d_dgrad_bf16
  return dgrad_phase_rows(dy, N, OH, OW, Kp, K, w_kcrs, C, R, S, stride, pad, dx, H, W, ws, ws_bytes, kRowConv,
                          as_stream(stream));
}

// Weight gradient: dw[k][c][r][s] = sum_{n,oh,ow} dy[n,oh,ow,k] * bn(x)[n, oh*stride + r - pad, ow*stride + s - pad, c]
// (+ l2 * w), split-K over the pixels into fp32 slabs, then the fixed-order reduce that also drops
// the channel padding (Cp -> C): wgrad() with bf16 operands and their own split rule.
DK_API size_t dk_conv2d_wgrad_bf16_workspace_bytes(int N, int OH, int OW, int K, int Cp, int R, int S) {
  return splitk_ws_bytes(K, R * S * Cp, N * OH * OW, kMfBf16);
}

namespace dk {
static inline bool wgrad_h_ok(const bf16_t* dy, const bf16_t* x, int N, int H, int W, int Cp, int C, int K, int R,
                              int S, int stride, const float* dw, const void* ws) {
  return Cp >= 4 && Cp % 4 == 0 && C >= 1 && C <= Cp && K >= 4 && K % 4 == 0 && N >= 1 && R >= 1 && S >= 1 &&
         stride >= 1 && al8(x) && al8(dy) && dw && aligned16(ws) && fits((size_t)N * H * W * Cp * 4);
}
}  // namespace dk

DK_API int dk_conv2d_wgrad_bf16(const bf16_t* dy, const bf16_t* x, int N, int H, int W, int Cp, int C, int K, int R,
                                int S, int stride, int pad, int OH, int OW, const float* w_kcrs, float l2,
                                float* dw_kcrs, void* ws, size_t ws_bytes, void* stream) {
  if (!wgrad_h_ok(dy, x, N, H, W, Cp, C, K, R, S, stride, dw_kcrs, ws)) return DK_ERR_ARGS;
  return wgrad(dy, img(x, N, H, W, Cp, OH, OW, R, S, stride, 1, -pad, N * OH * OW), K, R * S * Cp, w_kcrs, l2,
               dw_kcrs, 1, C, Cp, R, S, ws, ws_bytes, stream);
}

DK_API int dk_conv2d_wgrad_bnx_bf16(const bf16_t* dy, const bf16_t* x, int N, int H, int W, int Cp, int C, int K,
                                    int R, int S, int stride, int pad, int OH, int OW, const float* w_kcrs, float l2,
                                    float* dw_kcrs, void* ws, size_t ws_bytes, const float* bn_mean,
                                    const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                                    void* stream) {
  if (!wgrad_h_ok(dy, x, N, H, W, Cp, C, K, R, S, stride, dw_kcrs, ws)) return DK_ERR_ARGS;
  if (!bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta)) return DK_ERR_ARGS;
  return wgrad(dy,
               with_bn(img(x, N, H, W, Cp, OH, OW, R, S, stride, 1, -pad, N * OH * OW), bn_mean, bn_invstd, bn_gamma,
                       bn_beta, bn_relu),
               K, R * S * Cp, w_kcrs, l2, dw_kcrs, 1, C, Cp, R, S, ws, ws_bytes, stream);
}
