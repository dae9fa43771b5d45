// LeakyReLu, ReLu6, HardSwish and SiLu (layers/activations.py), gfx950: the
// plain forward, the forward with BatchNorm on load, and the plain backward.  The backward that also
// writes stage 1 of the preceding BatchNorm's backward (dk_act_bwd_bnx_*) lives in batchnorm.hip beside
// dk_relu_bwd_bn_partial_*, whose row geometry it shares.  The arithmetic is act_math.h's.
//
// No mask is stored: the backward recomputes act'(v) from the layer's input.  Memory-bound streaming
// kernels: a thread owns groups of eight consecutive elements (fp32: two 16-byte accesses per operand,
// bf16: one), the grid is capped at kActMaxBlocks blocks and strides over the rest.  The thread that
// meets the n % 8 tail takes it element by element, and so does every thread when a pointer is not
// 16-byte aligned (fp32 only; bf16 returns DK_ERR_ARGS as its siblings do).  With BatchNorm on load
// (_bnx) every loaded value goes through bn_in4 / bn_relu_out -- dk_bn_apply_*'s arithmetic -- and, for
// bf16 storage, is rounded to bf16 before the activation: bit-identical to dk_bn_apply_* followed by
// the plain entry.  Every output element is written exactly once.
#include "act_math.h"
#include "dk_common.h"

namespace dk {

constexpr int kActMaxBlocks = 2048;  // 256 CUs x 8 blocks of 256 threads

enum ActMode : int { kActFwd = 0, kActFwdBn = 1, kActBwd = 2 };

__device__ __forceinline__ f32x4 act_fwd4(int kind, float alpha, f32x4 v) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = act_fwd(kind, alpha, v[e]);
  return o;
}
__device__ __forceinline__ f32x4 act_grad4(int kind, float alpha, f32x4 v, f32x4 dy) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = act_grad(kind, alpha, v[e], dy[e]);
  return o;
}

// eight elements at p as two groups of four fp32 values (one 16-byte access for bf16, two for fp32)
template <class E>
__device__ __forceinline__ void ld8(const E* p, f32x4& lo, f32x4& hi) {
  if constexpr (sizeof(E) == 2) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    lo = bf16x4_to_f32(uint2{u.x, u.y});
    hi = bf16x4_to_f32(uint2{u.z, u.w});
  } else {
    lo = ld4(p);
    hi = ld4(p + 4);
  }
}
template <class E>
__device__ __forceinline__ void st8(E* p, f32x4 lo, f32x4 hi) {
  if constexpr (sizeof(E) == 2) {
    const uint2 a = f32_to_bf16x4(lo), c = f32_to_bf16x4(hi);
    *reinterpret_cast<uint4*>(p) = uint4{a.x, a.y, c.x, c.y};
  } else {
    st4(p, lo);
    st4(p + 4, hi);
  }
}

// out[k] for k in [0, n):  kActFwd act(x[k]);  kActFwdBn act(BN(x[k]) [+ ReLU]), the channel of element k
// being k % C;  kActBwd dy[k] * act'(x[k]).  VEC: every pointer is 16-byte aligned (and, with BN,
// C % 4 == 0 and the parameters aligned too).
template <class E, int MODE, bool VEC>
__global__ __launch_bounds__(256) void act_kernel(const E* __restrict__ x, const E* __restrict__ dy, long long n,
                                                  int C, BnIn bn, int kind, float alpha, E* __restrict__ out) {
  const long long groups = (n + 7) >> 3;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < groups; t += stride) {
    const long long k0 = t * 8;
    // the channel of the group's first element (a 64-bit remainder only for a buffer past 2^32 elements)
    int c0 = 0;
    if constexpr (MODE == kActFwdBn) c0 = (n >> 32) == 0 ? (int)((uint32_t)k0 % (uint32_t)C) : (int)(k0 % C);
    if (VEC && n - k0 >= 8) {
      f32x4 lo, hi;
      ld8(x + k0, lo, hi);
      if constexpr (MODE == kActFwdBn) {
        // C % 4 == 0 and k0 % 8 == 0: a group of four channels never wraps
        const int c1 = c0 + 4 == C ? 0 : c0 + 4;
        lo = rnd4<E>(bn_in4(lo, ld4(bn.mean + c0), ld4(bn.invstd + c0), ld4(bn.gamma + c0), ld4(bn.beta + c0), bn.relu));
        hi = rnd4<E>(bn_in4(hi, ld4(bn.mean + c1), ld4(bn.invstd + c1), ld4(bn.gamma + c1), ld4(bn.beta + c1), bn.relu));
      }
      if constexpr (MODE == kActBwd) {
        f32x4 glo, ghi;
        ld8(dy + k0, glo, ghi);
        st8(out + k0, act_grad4(kind, alpha, lo, glo), act_grad4(kind, alpha, hi, ghi));
      } else {
        st8(out + k0, act_fwd4(kind, alpha, lo), act_fwd4(kind, alpha, hi));
      }
      continue;
    }
    const int cnt = n - k0 >= 8 ? 8 : (int)(n - k0);
    int c = c0;
    for (int j = 0; j < cnt; ++j) {
      float v = ld1(x + k0 + j);
      if constexpr (MODE == kActFwdBn) {
        v = rnd1<E>(bn_relu_out(v, bn.mean[c], bn.invstd[c], bn.gamma[c], bn.beta[c], bn.relu));
        c = c + 1 == C ? 0 : c + 1;
      }
      if constexpr (MODE == kActBwd)
        st1(out + k0 + j, act_grad(kind, alpha, v, ld1(dy + k0 + j)));
      else
        st1(out + k0 + j, act_fwd(kind, alpha, v));
    }
  }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static inline bool act_kind_ok(int kind, float alpha) {
  return kind >= 0 && kind < kNumActKinds && alpha == alpha && alpha - alpha == 0.f;  // alpha finite
}

template <class E, int MODE>
static int act_t(const E* x, const E* dy, long long n, int C, const BnIn& bn, int kind, float alpha, E* out,
                 void* stream) {
  if (!x || !out || n < 1 || !act_kind_ok(kind, alpha)) return DK_ERR_ARGS;
  if (MODE == kActBwd && !dy) return DK_ERR_ARGS;
  if (MODE == kActFwdBn && (C < 1 || n % C != 0 || !bn.mean || !bn.invstd || !bn.gamma || !bn.beta)) return DK_ERR_ARGS;
  bool vec = aligned16(x) && aligned16(out) && (MODE != kActBwd || aligned16(dy));
  if (MODE == kActFwdBn)
    vec = vec && C % 4 == 0 && aligned16(bn.mean) && aligned16(bn.invstd) && aligned16(bn.gamma) && aligned16(bn.beta);
  if (!vec && sizeof(E) != 4) return DK_ERR_ARGS;
  const long long blocks = cdivll(cdivll(n, 8), 256);
  const dim3 grid((unsigned)(blocks < kActMaxBlocks ? blocks : kActMaxBlocks));
  if (vec)
    hipLaunchKernelGGL((act_kernel<E, MODE, true>), grid, dim3(256), 0, as_stream(stream), x, dy, n, C, bn, kind, alpha,
                       out);
  else
    hipLaunchKernelGGL((act_kernel<E, MODE, false>), grid, dim3(256), 0, as_stream(stream), x, dy, n, C, bn, kind,
                       alpha, out);
  return launch_status();
}

static const BnIn kNoBn = BnIn{nullptr, nullptr, nullptr, nullptr, 0};

}  // namespace dk

using namespace dk;

DK_API int dk_act_fwd_f32(const float* x, long long n, int kind, float alpha, float* y, void* stream) {
  return act_t<float, kActFwd>(x, nullptr, n, 1, kNoBn, kind, alpha, y, stream);
}
DK_API int dk_act_fwd_bf16(const uint16_t* x, long long n, int kind, float alpha, uint16_t* y, void* stream) {
  return act_t<bf16_t, kActFwd>(x, nullptr, n, 1, kNoBn, kind, alpha, y, stream);
}
DK_API int dk_act_fwd_bnx_f32(const float* x, long long n, int C, const float* bn_mean, const float* bn_invstd,
                              const float* bn_gamma, const float* bn_beta, int bn_relu, int kind, float alpha, float* y,
                              void* stream) {
  return act_t<float, kActFwdBn>(x, nullptr, n, C, BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, kind, alpha, y,
                                 stream);
}
DK_API int dk_act_fwd_bnx_bf16(const uint16_t* x, long long n, int C, const float* bn_mean, const float* bn_invstd,
                               const float* bn_gamma, const float* bn_beta, int bn_relu, int kind, float alpha,
                               uint16_t* y, void* stream) {
  return act_t<bf16_t, kActFwdBn>(x, nullptr, n, C, BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, kind, alpha,
                                  y, stream);
}
DK_API int dk_act_bwd_f32(const float* x, const float* dy, long long n, int kind, float alpha, float* dx, void* stream) {
  return act_t<float, kActBwd>(x, dy, n, 1, kNoBn, kind, alpha, dx, stream);
}
DK_API int dk_act_bwd_bf16(const uint16_t* x, const uint16_t* dy, long long n, int kind, float alpha, uint16_t* dx,
                           void* stream) {
  return act_t<bf16_t, kActBwd>(x, dy, n, 1, kNoBn, kind, alpha, dx, stream);
}
