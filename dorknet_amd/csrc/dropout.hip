// Dropout with a counter-based mask, gfx950.  No layer of the reference: an
// extension (layers/dropout.py).
//
// The keep bit of an element is a pure function of (seed, step, lane, element index), so nothing is
// stored between the passes: the backward regenerates the mask, and the layer costs one read and one
// write per pass.  Generator: Philox4x32-10 (Salmon et al., Random123) in plain C++.  Element i is the
// linear index in storage order plus the buffer's first_index; block b = i >> 3 shares one Philox call
//   counter = (b & 0xffffffff, b >> 32, step & 0xffffffff, lane),  key = (seed & 0xffffffff, seed >> 32)
// and with j = i & 7 the element's 16-bit field is output word j >> 1, low half for even j, high half
// for odd j.  The element is kept iff field >= threshold (= floor(p * 65536)); a kept element is
// x * scale with scale = fp32(65536 / (65536 - threshold)), one fp32 rounding (bf16 storage: the fp32
// product rounded to nearest even once); a dropped element is +0.0 whatever x was.
//
// One thread owns one block of eight elements: one Philox call, 32 bytes (fp32: two 16-byte accesses)
// or 16 bytes (bf16: one) loaded and stored.  first_index is a multiple of 8, so Philox blocks start
// on the buffer's first element.  The last thread takes the n % 8 tail element by element, and so
// does every thread when a pointer is not 16-byte aligned.  With BN on load (_bnx) every loaded value
// goes through bn_in4 / bn_relu_out -- dk_bn_apply_*'s arithmetic -- and, for bf16 storage, is rounded
// to bf16 before the mask: bit-identical to dk_bn_apply_* followed by the plain entry.
#include "dk_common.h"

namespace dk {

struct Philox {
  uint32_t w[4];
};

__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox{{c0, c1, c2, c3}};
}

__device__ __forceinline__ bool kept(const Philox& r, int j, uint32_t threshold) {
  return ((r.w[j >> 1] >> (16 * (j & 1))) & 0xffffu) >= threshold;
}

// elements j0..j0+3 of the block: keep ? v * scale : +0.0
__device__ __forceinline__ f32x4 mask4(f32x4 v, const Philox& r, int j0, uint32_t threshold, float scale) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = kept(r, j0 + e, threshold) ? v[e] * scale : 0.f;
  return o;
}

// y[k] = keep(first_index + k) ? f(x[k]) * scale : +0.0 for k in [0, n); f = BN (+ ReLU) on load or the
// identity.  VEC: x and y are 16-byte aligned (and, with BN, C % 4 == 0 and the parameters aligned).
template <class E, bool BN, bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(const E* x, long long n, uint32_t threshold, float scale,
                                                      uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t lane,
                                                      long long first_block, int C, BnIn bn, E* y) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long k0 = t * 8;
  if (k0 >= n) return;
  const unsigned long long b = (unsigned long long)(first_block + t);
  // the channel of the thread's first element (a 64-bit remainder only for a buffer past 2^32 elements)
  int c0 = 0;
  if constexpr (BN) c0 = (n >> 32) == 0 ? (int)((uint32_t)k0 % (uint32_t)C) : (int)(k0 % C);
  if (VEC && n - k0 >= 8) {
    f32x4 lo, hi;  // (the loads are issued before the generator's forty multiplies)
    if constexpr (sizeof(E) == 2) {
      const uint4 u = *reinterpret_cast<const uint4*>(x + k0);
      lo = bf16x4_to_f32(uint2{u.x, u.y});
      hi = bf16x4_to_f32(uint2{u.z, u.w});
    } else {
      lo = ld4(x + k0);
      hi = ld4(x + k0 + 4);
    }
    const Philox r = philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), step, lane, seed_lo, seed_hi);
    if constexpr (BN) {
      // C % 4 == 0 and k0 % 8 == 0: a group of four channels never wraps
      const int c1 = c0 + 4 == C ? 0 : c0 + 4;
      lo = rnd4<E>(bn_in4(lo, ld4(bn.mean + c0), ld4(bn.invstd + c0), ld4(bn.gamma + c0), ld4(bn.beta + c0), bn.relu));
      hi = rnd4<E>(bn_in4(hi, ld4(bn.mean + c1), ld4(bn.invstd + c1), ld4(bn.gamma + c1), ld4(bn.beta + c1), bn.relu));
    }
    lo = mask4(lo, r, 0, threshold, scale);
    hi = mask4(hi, r, 4, threshold, scale);
    if constexpr (sizeof(E) == 2) {
      const uint2 a = f32_to_bf16x4(lo), c = f32_to_bf16x4(hi);
      *reinterpret_cast<uint4*>(y + k0) = uint4{a.x, a.y, c.x, c.y};
    } else {
      st4(y + k0, lo);
      st4(y + k0 + 4, hi);
    }
    return;
  }
  const Philox r = philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), step, lane, seed_lo, seed_hi);
  const int cnt = n - k0 >= 8 ? 8 : (int)(n - k0);
  int c = c0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j < cnt) {
      float v = ld1(x + k0 + j);
      if constexpr (BN) {
        v = rnd1<E>(bn_relu_out(v, bn.mean[c], bn.invstd[c], bn.gamma[c], bn.beta[c], bn.relu));
        c = c + 1 == C ? 0 : c + 1;
      }
      st1(y + k0 + j, kept(r, j, threshold) ? v * scale : 0.f);
    }
  }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <class E, bool BN>
static int dropout_t(const E* x, long long n, int threshold, long long seed, long long step, int lane,
                     long long first_index, int C, const BnIn& bn, E* y, void* stream) {
  if (!x || !y || n < 1 || threshold < 0 || threshold > 65535 || seed < 0 || step < 0 || lane < 0 ||
      first_index < 0 || (first_index & 7) != 0)
    return DK_ERR_ARGS;
  if (first_index > 0x7fffffffffffffffll - n) return DK_ERR_ARGS;  // the last element's index fits 63 bits
  if (BN && (C < 1 || !bn.mean || !bn.invstd || !bn.gamma || !bn.beta)) return DK_ERR_ARGS;
  // the reciprocal of the probability actually realised; both operands are exact in fp32, so the
  // division is correctly rounded
  const float scale = 65536.f / (float)(65536 - threshold);
  const long long threads = cdivll(n, 8);  // one block of eight elements each: the grid follows n
  if (cdivll(threads, 256) > 0x7fffffffll) return DK_ERR_ARGS;
  const dim3 grid((unsigned)cdivll(threads, 256));
  bool vec = aligned16(x) && aligned16(y);
  if (BN)
    vec = vec && C % 4 == 0 && aligned16(bn.mean) && aligned16(bn.invstd) && aligned16(bn.gamma) && aligned16(bn.beta);
  const unsigned long long s = (unsigned long long)seed;
#define DK_DROPOUT(VEC)                                                                                          \
  hipLaunchKernelGGL((dropout_kernel<E, BN, VEC>), grid, dim3(256), 0, as_stream(stream), x, n, (uint32_t)threshold, \
                     scale, (uint32_t)s, (uint32_t)(s >> 32), (uint32_t)((unsigned long long)step & 0xffffffffull), \
                     (uint32_t)lane, first_index >> 3, C, bn, y)
  if (vec) DK_DROPOUT(true);
  else DK_DROPOUT(false);
#undef DK_DROPOUT
  return launch_status();
}

static const BnIn kNoBn = BnIn{nullptr, nullptr, nullptr, nullptr, 0};

}  // namespace dk

using namespace dk;

DK_API int dk_dropout_fwd_f32(const float* x, long long n, int threshold, long long seed, long long step, int lane,
                              long long first_index, float* y, void* stream) {
  return dropout_t<float, false>(x, n, threshold, seed, step, lane, first_index, 1, kNoBn, y, stream);
}
DK_API int dk_dropout_fwd_bf16(const uint16_t* x, long long n, int threshold, long long seed, long long step, int lane,
                               long long first_index, uint16_t* y, void* stream) {
  return dropout_t<bf16_t, false>(x, n, threshold, seed, step, lane, first_index, 1, kNoBn, y, stream);
}
DK_API int dk_dropout_fwd_bnx_f32(const float* x, long long n, int threshold, long long seed, long long step, int lane,
                                  long long first_index, int C, const float* bn_mean, const float* bn_invstd,
                                  const float* bn_gamma, const float* bn_beta, int bn_relu, float* y, void* stream) {
  return dropout_t<float, true>(x, n, threshold, seed, step, lane, first_index, C,
                                BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, y, stream);
}
DK_API int dk_dropout_fwd_bnx_bf16(const uint16_t* x, long long n, int threshold, long long seed, long long step,
                                   int lane, long long first_index, int C, const float* bn_mean,
                                   const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                                   uint16_t* y, void* stream) {
  return dropout_t<bf16_t, true>(x, n, threshold, seed, step, lane, first_index, C,
                                 BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, y, stream);
}
// dx = keep ? dy * scale : +0.0: the plain forward's kernel over dy
DK_API int dk_dropout_bwd_f32(const float* dy, long long n, int threshold, long long seed, long long step, int lane,
                              long long first_index, float* dx, void* stream) {
  return dropout_t<float, false>(dy, n, threshold, seed, step, lane, first_index, 1, kNoBn, dx, stream);
}
DK_API int dk_dropout_bwd_bf16(const uint16_t* dy, long long n, int threshold, long long seed, long long step, int lane,
                               long long first_index, uint16_t* dx, void* stream) {
  return dropout_t<bf16_t, false>(dy, n, threshold, seed, step, lane, first_index, 1, kNoBn, dx, stream);
}
