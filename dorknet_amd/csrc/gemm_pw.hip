// Pointwise (1x1) convolution entry points (layers/pointwise_convolution.py) on the implicit-GEMM
// engine (gemm_engine.h) and the streaming kernels (pw_stream.hip).
#include "gemm_engine.h"
#include "pw_launch.h"

using namespace dk;

// The path of the forward (dk_pwconv_fwd_stats_rows, dk_pwconv_fwd_ex_f32) and of the dgrad with the
// following BatchNorm's backward on load (dk_pwconv_dgrad_bnbwd_stats_rows, dk_pwconv_dgrad_bnbwd_f32,
// and dk_pwconv_dgrad_f32's plain form, deep only).
//
// Launch-only conditions (what the row queries cannot see; DESIGN.md lists them):
//   * xbytes: the queries pass 0, the launch the input's real extent -- which dk_pwconv_fwd_ex_f32 has
//     already held below 2 GiB (fits), so the two choices agree;
//   * a given input BatchNorm that is incomplete or misaligned (bn_ok): the deep paths refuse the
//     call; the streaming forward leaves it to the tiled engine, which refuses it too.
// So no fp32 call reaches a path whose row count differs from the query's.
static PwChoice pw_fwd_choice(int M, int K, int C, size_t xbytes) {
  return pw_choice(pw_deep_fwd_plan(M, K, C, xbytes), pw_stream_fwd_plan(M, K, C, xbytes));
}
static PwChoice pw_dgrad_choice(int M, int K, int C) {
  return pw_choice(pw_deep_dgrad_plan(M, K, C), pw_stream_dgrad_plan(M, K, C));
}

// y[n,oh,ow,k] = sum_c x[n, oh*s, ow*s, c] * w[k][c] (+ bias)
DK_API int dk_pwconv_fwd_f32(const float* x, int N, int H, int W, int C, const float* w_kc, int K, int stride,
                             const float* bias, float* y, int OH, int OW, void* stream) {
  if (!fits((size_t)N * H * W * C * 4)) return DK_ERR_ARGS;
  if (C % 4 == 0 && aligned16(x) && aligned16(w_kc)) {
    // the deep streaming kernel (pw_deep.hip), bit-identical y (the strided skip projections)
    const PwPlan deep = pw_deep_fwd_plan(N * OH * OW, K, C, (size_t)N * H * W * C * 4);
    if (deep.rows)
      return pw_deep_fwd(x, N, H, W, stride, OH, OW, w_kc, K, C, bias, y, nullptr, nullptr, nullptr, nullptr, 0,
                         nullptr, deep, as_stream(stream));
  }
  if (C % 4 || !aligned16(x) || !aligned16(w_kc)) {
    // Unaligned channel count: scalar loads, stride 1 only (the rows are then a plain matrix).
    if (stride != 1) return DK_ERR_ARGS;
    return igemm_rows<LdMatKC1, LdMatKC1>(mat(x, N * H * W, C, N * H * W), mat(w_kc, K, C, K), ep_store(y, K, bias),
                                          N * H * W, K, C, kRowPlain, as_stream(stream));
  }
  return fwd_rows(img1(x, N, H, W, C, OH, OW, stride, N * OH * OW), w_kc, K, C, bias, y, nullptr, nullptr, nullptr,
                  nullptr, 0, nullptr, kRowPlain, as_stream(stream));
}

// The same with x = the raw output of the previous layer and y = pw(bn(x)) (+ReLU inside).
DK_API int dk_pwconv_fwd_bnx_f32(const float* x, int N, int H, int W, int C, const float* w_kc, int K, int stride,
                                 const float* bias, float* y, int OH, int OW, const float* bn_mean,
                                 const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                                 void* stream) {
  if (C % 4 || !aligned16(x) || !aligned16(w_kc) || !fits((size_t)N * H * W * C * 4)) return DK_ERR_ARGS;
  if (!bn_mean) return DK_ERR_ARGS;  // (to the body NULL means no input BatchNorm)
  return fwd_rows(img1(x, N, H, W, C, OH, OW, stride, N * OH * OW), w_kc, K, C, bias, y, bn_mean, bn_invstd, bn_gamma,
                  bn_beta, bn_relu, nullptr, kRowPlain, as_stream(stream));
}

DK_API int dk_pwconv_fwd_stats_rows(int N, int OH, int OW, int K, int C) {
  const int M = N * OH * OW;
  const PwChoice c = pw_fwd_choice(M, K, C, 0);
  return c.path == kPwTiled ? stats_rows(M, K, C) : c.plan.rows;
}

DK_API int dk_pwconv_fwd_ex_f32(const float* x, int N, int H, int W, int C, const float* w_kc, int K, int stride,
                                const float* bias, float* y, int OH, int OW, const float* bn_mean,
                                const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                                double* stats, void* stream) {
  if (C % 4 || !aligned16(x) || !aligned16(w_kc) || !fits((size_t)N * H * W * C * 4)) return DK_ERR_ARGS;
  const PwChoice c = pw_fwd_choice(N * OH * OW, K, C, (size_t)N * H * W * C * 4);
  if (c.path == kPwDeep) {
    // the deep streaming kernel (pw_deep.hip): bit-identical y, its own partial rows and slices
    // (dk_pwconv_fwd_stats_rows sized the partials for it: no other path may take this call)
    if (bn_mean && !bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta)) return DK_ERR_ARGS;
    return pw_fold_launch(stats, c.plan, K, [&](const FoldTail* ft) {
      return pw_deep_fwd(x, N, H, W, stride, OH, OW, w_kc, K, C, bias, y, bn_mean, bn_invstd, bn_gamma, bn_beta,
                         bn_relu, stats, c.plan, as_stream(stream), ft);
    });
  }
  if (c.path == kPwStream && (!bn_mean || bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta)))
    // K = C = 64 / 128: the persistent streaming kernel (pw_stream.hip), bit-identical outputs
    return pw_fold_launch(stats, c.plan, K, [&](const FoldTail* ft) {
      return pw_stream_fwd(x, N, H, W, stride, OH, OW, w_kc, K, bias, y, bn_mean, bn_invstd, bn_gamma, bn_beta,
                           bn_relu, stats, c.plan, as_stream(stream), ft);
    });
  // kRowPlain: the fp32 pointwise forward picks its tile as a plain GEMM (the bf16 twin as kRowFwdH)
  return fwd_rows(img1(x, N, H, W, C, OH, OW, stride, N * OH * OW), w_kc, K, C, bias, y, bn_mean, bn_invstd, bn_gamma,
                  bn_beta, bn_relu, stats, kRowPlain, as_stream(stream));
}

// Pointwise dgrad (pointwise_convolution.py:65-72): dx_rows = dy_rows . W; for stride > 1 the
// result is widened to (OH*s, OW*s) with zeros off the sampling lattice.
DK_API int dk_pwconv_dgrad_f32(const float* dy, int N, int OH, int OW, int K, const float* w_kc, int C, int stride,
                               float* dx, void* stream) {
  const int M = N * OH * OW;
  if (!fits((size_t)M * K * 4)) return DK_ERR_ARGS;
  const hipStream_t st = as_stream(stream);
  if (stride == 1 && vec_ok(mat(dy, M, K, M), K, 4) && vec_ok(mat(w_kc, K, C, C), 4, C) && aligned16(dy) &&
      aligned16(w_kc) && aligned16(dx)) {
    // the deep dgrad kernel's plain form (pw_deep.hip): bit-identical dx (the skip projections)
    const PwPlan deep = pw_deep_dgrad_plan(M, K, C);
    if (deep.rows) return pw_deep_dgrad_plain(dy, M, K, C, w_kc, dx, deep, st);
  }
  return pw_dgrad_tail<float>(dy, M, OH, OW, K, w_kc, C, stride, dx, nullptr, nullptr, BnIn{}, nullptr, st);
}

DK_API int dk_pwconv_dgrad_stats_rows(int N, int OH, int OW, int K, int C) { return stats_rows(N * OH * OW, C, K); }
DK_API int dk_pwconv_dgrad_bnbwd_stats_rows(int N, int OH, int OW, int K, int C) {
  const int M = N * OH * OW;
  const PwChoice c = pw_dgrad_choice(M, K, C);
  return c.path == kPwTiled ? stats_rows(M, C, K, kRowBnBwd) : c.plan.rows;
}

// dgrad + the BN-backward partial sums of the BatchNorm whose output this layer consumed
// (bn_x = that BN's raw input, on the dx grid; part: dk_pwconv_dgrad_stats_rows() x 2 x C).
DK_API int dk_pwconv_dgrad_ex_f32(const float* dy, int N, int OH, int OW, int K, const float* w_kc, int C, int stride,
                                  float* dx, const float* residual, const float* bn_x, const float* bn_mean,
                                  const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                                  double* part, void* stream) {
  const int M = N * OH * OW;
  if (!fits((size_t)M * K * 4) || (part != nullptr) != (bn_x != nullptr)) return DK_ERR_ARGS;
  if (part && (!bn_mean || !bn_invstd || !bn_gamma || !bn_beta)) return DK_ERR_ARGS;
  if (part && residual && stride != 1) return DK_ERR_ARGS;  // off-lattice residual terms would need reducing
  // (any alignment of bn_x and of the BN vectors is taken: v4 drops to the scalar partial loads)
  return pw_dgrad_tail(dy, M, OH, OW, K, w_kc, C, stride, dx, residual, bn_x,
                       BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, part, as_stream(stream));
}

// dk_pwconv_dgrad_ex_f32 with the input BN's partials for stride > 1, the widened gradient kept
// compact (EpLatticeBnBwd): dx_lat[n][oh][ow][c] = the widened dx at (n, s*oh, s*ow, c), the
// rest of the widened grid being zero; part has dk_pwconv_dgrad_stats_rows() rows.
DK_API int dk_pwconv_dgrad_lattice_f32(const float* dy, int N, int OH, int OW, int K, const float* w_kc, int C,
                                       int stride, float* dx_lat, const float* bn_x, const float* bn_mean,
                                       const float* bn_invstd, const float* bn_gamma, const float* bn_beta,
                                       int bn_relu, double* part, void* stream) {
  const int M = N * OH * OW;
  if (!fits((size_t)M * K * 4) || !fits((size_t)M * C * 4) || stride < 2 || !dx_lat || !bn_x || !part)
    return DK_ERR_ARGS;
  if (!bn_mean || !bn_invstd || !bn_gamma || !bn_beta) return DK_ERR_ARGS;
  const BnIn bn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu};
  return pw_dgrad_rows(mat(dy, M, K, M), mat(w_kc, K, C, C),
                       ep_bnbwd<EpLatticeBnBwd>(ep_widen(dx_lat, C, OH, OW, stride), part, bn_x, bn), M, C, K,
                       as_stream(stream));
}

// dgrad of a stride-1 pointwise layer whose output fed a BatchNorm (+ReLU), with that BN's
// backward apply (dk_bn_bwd_apply_f32) done on load: g = the gradient w.r.t. the BN(+ReLU)
// output, bn_x = the BN's raw input (= this layer's output), k12 from
// dk_bn_bwd_from_partials_f32.  dy_out (nullable) receives dy = the gradient w.r.t. bn_x,
// bit-identical to dk_bn_bwd_apply_f32's, for this layer's weight gradient.  The epilogue
// options (residual, the partials of the BN before this layer) are those of
// dk_pwconv_dgrad_ex_f32 at stride 1; part has dk_pwconv_dgrad_bnbwd_stats_rows() rows.
DK_API int dk_pwconv_dgrad_bnbwd_f32(const float* g, const float* bn_x, int N, int OH, int OW, int K,
                                     const float* out_mean, const float* out_invstd, const float* out_gamma,
                                     const float* out_beta, int out_relu, const float* k12, float* dy_out,
                                     const float* w_kc, int C, float* dx, const float* residual, const float* x,
                                     const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                     const float* bn_beta, int bn_relu, double* part, void* stream) {
  const int M = N * OH * OW;
  if (!fits((size_t)M * K * 4) || (part != nullptr) != (x != nullptr)) return DK_ERR_ARGS;
  if (part && (!bn_mean || !bn_invstd || !bn_gamma || !bn_beta)) return DK_ERR_ARGS;
  if (!out_mean || !out_invstd || !out_gamma || !out_beta || !k12 || !bn_x) return DK_ERR_ARGS;
  const hipStream_t st = as_stream(stream);
  // 16-byte loads of g, bn_x and dy_out; the LDS table holds 2 float4 per channel
  if (!vec_ok(mat(w_kc, K, C, C), 4, C) || K % 4 || !aligned16(g) || !aligned16(bn_x) || (dy_out && !aligned16(dy_out)) ||
      (size_t)K * 32 > 64 * 1024)
    return DK_ERR_ARGS;
  const PwChoice c = pw_dgrad_choice(M, K, C);
  if (c.path != kPwTiled) {
    // the deep streaming kernel (pw_deep.hip) or, at K = C = 64, the persistent streaming kernel
    // (pw_stream.hip): bit-identical dy and dx, their own partial rows (sized by
    // dk_pwconv_dgrad_bnbwd_stats_rows: no other path may take this call)
    if (part && !bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta)) return DK_ERR_ARGS;
    return pw_fold_launch(part, c.plan, C, [&](const FoldTail* ft) {
      if (c.path == kPwDeep)
        return pw_deep_dgrad_bnbwd(g, bn_x, M, K, C, out_mean, out_invstd, out_gamma, out_beta, out_relu, k12, dy_out,
                                   w_kc, dx, residual, part ? x : nullptr, bn_mean, bn_invstd, bn_gamma, bn_beta,
                                   bn_relu, part, c.plan, st, ft);
      return pw_stream_dgrad_bnbwd(g, bn_x, M, out_mean, out_invstd, out_gamma, out_beta, out_relu, k12, dy_out, w_kc,
                                   dx, residual, part ? x : nullptr, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu,
                                   part, c.plan, st, ft);
    });
  }
  // (with part, any alignment of x and of the BN vectors is taken: v4 drops to the scalar partial loads)
  return pw_dgrad_bnbwd_tail(
      with_bnbwd(mat(g, M, K, M), bn_x, BnBwdIn{out_mean, out_invstd, out_gamma, out_beta, k12, out_relu, K}, dy_out), M, K,
      w_kc, C, dx, residual, x, BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, part, st);
}

DK_API size_t dk_pwconv_wgrad_workspace_bytes(int N, int OH, int OW, int K, int C) {
  // (one query for both dtypes' entries; the bf16 twin's tiles can differ: the larger of the two needs)
  const int M = N * OH * OW;
  size_t a = splitk_ws_bytes(K, C, M), b = splitk_ws_bytes(K, C, M, kMfBf16);
  if (a < b) a = b;
  return a;
}

// dw[k][c] = sum_{n,oh,ow} dy[n,oh,ow,k] * x[n, oh*s, ow*s, c]  (+ l2 * w)   (pointwise_convolution.py:61-64)
DK_API int dk_pwconv_wgrad_f32(const float* dy, const float* x, int N, int H, int W, int C, int K, int stride,
                               int OH, int OW, const float* w_kc, float l2, float* dw_kc, void* ws, size_t ws_bytes,
                               void* stream) {
  if (C % 4 || !aligned16(x) || !fits((size_t)N * H * W * C * 4)) return DK_ERR_ARGS;
  const int M = N * OH * OW;
  return wgrad(dy, img(x, N, H, W, C, OH, OW, 1, 1, stride, 1, 0, M), K, C, w_kc, l2, dw_kc, 0, C, C, 1, 1,
               ws, ws_bytes, stream);
}

DK_API int dk_pwconv_wgrad_bnx_f32(const float* dy, const float* x, int N, int H, int W, int C, int K, int stride,
                                   int OH, int OW, const float* w_kc, float l2, float* dw_kc, void* ws,
                                   size_t ws_bytes, const float* bn_mean, const float* bn_invstd,
                                   const float* bn_gamma, const float* bn_beta, int bn_relu, void* stream) {
  if (C % 4 || !aligned16(x) || !fits((size_t)N * H * W * C * 4)) return DK_ERR_ARGS;
  if (!bn_ok(bn_mean, bn_invstd, bn_gamma, bn_beta)) return DK_ERR_ARGS;
  return wgrad(dy,
               with_bn(img(x, N, H, W, C, OH, OW, 1, 1, stride, 1, 0, N * OH * OW), bn_mean, bn_invstd, bn_gamma,
                       bn_beta, bn_relu),
               K, C, w_kc, l2, dw_kc, 0, C, C, 1, 1, ws, ws_bytes, stream);
}

