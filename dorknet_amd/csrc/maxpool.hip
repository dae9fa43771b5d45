// Max pooling (layers/pooling.py:45-77, layers/pooling_cy.pyx:8-88 in the reference), gfx950.
//
// Window stride x stride, non-overlapping; OH = H / stride, OW = W / stride (floor): the trailing
// H % stride rows and W % stride columns are not pooled and receive a zero gradient.  The arg-max
// scans the window row-major from (0, 0) with a strict >, so the first maximum wins (pool_train).
//
// The operation is HBM-bound, so the design is bytes moved.  The reference keeps an int32 location
// map the size of the input (4 bytes per input element); here the training forward writes
// idx[N][OH][OW][C], one uint8 per *output* element holding m * stride + n (stride <= 16), and the
// backward writes every element of dx exactly once (dy or 0) from dy and idx: no memset, no atomics.
//
// One thread handles one output pixel times V channels (V = 4: 16-byte fp32 / 8-byte bf16 vectors,
// the four idx bytes as one 32-bit word; V = 1: any C, any alignment).  With BN on load (_bnx) every
// loaded value goes through bn_in4 / bn_relu_out -- dk_bn_apply_*'s arithmetic -- and, for bf16
// storage, is rounded to bf16 *before* the comparison: the unfused path pools round(bn(x)), and the
// rounding creates ties that a comparison in fp32 would resolve to a later location.
#include "dk_common.h"

namespace dk {

template <class E, int V>
struct PoolVec;
template <class E>
struct PoolVec<E, 4> {
  typedef f32x4 T;
  static __device__ __forceinline__ T load(const E* p) { return ld4(p); }
  static __device__ __forceinline__ T loadf(const float* p) { return ld4(p); }
  static __device__ __forceinline__ void store(E* p, T v) { st4(p, v); }
  static __device__ __forceinline__ T bn(T v, T m, T is, T g, T b, int relu) {
    return rnd4<E>(bn_in4(v, m, is, g, b, relu));
  }
  static __device__ __forceinline__ T zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ float get(T v, int e) { return v[e]; }
  static __device__ __forceinline__ void set(T& v, int e, float f) { v[e] = f; }
  static __device__ __forceinline__ uint32_t ldidx(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
  static __device__ __forceinline__ void stidx(uint8_t* p, uint32_t w) { *reinterpret_cast<uint32_t*>(p) = w; }
};
template <class E>
struct PoolVec<E, 1> {
  typedef float T;
  static __device__ __forceinline__ T load(const E* p) { return ld1(p); }
  static __device__ __forceinline__ T loadf(const float* p) { return *p; }
  static __device__ __forceinline__ void store(E* p, T v) { st1(p, v); }
  static __device__ __forceinline__ T bn(T v, T m, T is, T g, T b, int relu) {
    return rnd1<E>(bn_relu_out(v, m, is, g, b, relu));
  }
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ float get(T v, int) { return v; }
  static __device__ __forceinline__ void set(T& v, int, float f) { v = f; }
  static __device__ __forceinline__ uint32_t ldidx(const uint8_t* p) { return *p; }
  static __device__ __forceinline__ void stidx(uint8_t* p, uint32_t w) { *p = (uint8_t)w; }
};

// y[n][p][q][c] = max over the window, idx[n][p][q][c] = m * stride + n of the first maximum
// (idx == NULL: the test-mode forward).  S: the stride at compile time (all window loads in
// flight at once), 0 = any stride, taken from `stride`.
template <class E, int V, bool BN, int S>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const E* __restrict__ x, int H, int W, int C, int stride,
                                                          int OH, int OW, long long total, BnIn bn,
                                                          E* __restrict__ y, uint8_t* __restrict__ idx) {
  using PV = PoolVec<E, V>;
  typedef typename PV::T T;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int s = S ? S : stride;
  const int CV = C / V;
  const int cv = (int)(t % CV);
  long long r = t / CV;
  const int q = (int)(r % OW);
  r /= OW;
  const int p = (int)(r % OH);
  const long long n = r / OH;
  const int c0 = cv * V;
  T mu = PV::zero(), is = PV::zero(), ga = PV::zero(), be = PV::zero();
  if constexpr (BN) {
    mu = PV::loadf(bn.mean + c0);
    is = PV::loadf(bn.invstd + c0);
    ga = PV::loadf(bn.gamma + c0);
    be = PV::loadf(bn.beta + c0);
  }
  const E* xp = x + ((n * H + (long long)p * s) * W + (long long)q * s) * C + c0;
  const long long row = (long long)W * C;
  T best = PV::zero();
  uint32_t loc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) loc[e] = 0;
  auto take = [&](T v, int k) {
    if constexpr (BN) v = PV::bn(v, mu, is, ga, be, bn.relu);
    if (k == 0) {
      best = v;
      return;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float f = PV::get(v, e);
      if (f > PV::get(best, e)) {
        PV::set(best, e, f);
        loc[e] = (uint32_t)k;
      }
    }
  };
  if constexpr (S != 0) {
    T v[S * S];
#pragma unroll
    for (int m = 0; m < S; ++m)
#pragma unroll
      for (int j = 0; j < S; ++j) v[m * S + j] = PV::load(xp + m * row + (long long)j * C);
#pragma unroll
    for (int k = 0; k < S * S; ++k) take(v[k], k);
  } else {
    for (int m = 0; m < s; ++m)
      for (int j = 0; j < s; ++j) take(PV::load(xp + m * row + (long long)j * C), m * s + j);
  }
  const long long o = t * V;  // y and idx are [N][OH][OW][C]: the thread order is the element order
  PV::store(y + o, best);
  if (idx) {
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < V; ++e) w |= loc[e] << (8 * e);
    PV::stidx(idx + o, w);
  }
}

// dx[n][p*s + m][q*s + j][c] = (idx == m*s + j) ? dy[n][p][q][c] : 0, and 0 on the trailing rows and
// columns: the threads of the last output column clear the W % s columns beside their window, the
// threads of the last output row clear the H % s rows below theirs, and the corner goes with the
// last output row (its last thread's strip runs on to W).  Every dx element is written exactly once.
template <class E, int V, int S>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const E* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                          int H, int W, int C, int stride, int OH, int OW,
                                                          long long total, E* __restrict__ dx) {
  using PV = PoolVec<E, V>;
  typedef typename PV::T T;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int s = S ? S : stride;
  const int CV = C / V;
  const int cv = (int)(t % CV);
  long long r = t / CV;
  const int q = (int)(r % OW);
  r /= OW;
  const int p = (int)(r % OH);
  const long long n = r / OH;
  const int c0 = cv * V;
  const long long o = t * V;
  const T g = PV::load(dy + o);
  const uint32_t w = PV::ldidx(idx + o);
  E* img = dx + n * H * W * C + c0;
  const long long row = (long long)W * C;
  E* xp = img + (long long)p * s * row + (long long)q * s * C;
  auto put = [&](int m, int j) {
    T v = PV::zero();
    const uint32_t k = (uint32_t)(m * s + j);
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (((w >> (8 * e)) & 0xffu) == k) PV::set(v, e, PV::get(g, e));
    PV::store(xp + m * row + (long long)j * C, v);
  };
  if constexpr (S != 0) {
#pragma unroll
    for (int m = 0; m < S; ++m)
#pragma unroll
      for (int j = 0; j < S; ++j) put(m, j);
  } else {
    for (int m = 0; m < s; ++m)
      for (int j = 0; j < s; ++j) put(m, j);
  }
  const T z = PV::zero();
  if (q == OW - 1)  // the remainder columns beside this window's rows
    for (int h = p * s; h < p * s + s; ++h)
      for (int ww = OW * s; ww < W; ++ww) PV::store(img + h * row + (long long)ww * C, z);
  if (p == OH - 1) {  // the remainder rows below this window's columns (the last thread: on to W)
    const int w1 = (q == OW - 1) ? W : q * s + s;
    for (int h = OH * s; h < H; ++h)
      for (int ww = q * s; ww < w1; ++ww) PV::store(img + h * row + (long long)ww * C, z);
  }
}

// stride 1..16 (the location has to fit a byte), positive sizes, at least one output pixel
static inline bool pool_args_ok(int N, int H, int W, int C, int stride) {
  return stride >= 1 && stride <= 16 && N >= 1 && H >= 1 && W >= 1 && C >= 1 && H / stride >= 1 && W / stride >= 1;
}

// 4-channel vectors: C % 4 == 0 and every pointer aligned for its vector type
template <class E>
static inline bool pool_vec_ok(int C, const E* a, const E* b, const uint8_t* idx, const BnIn* bn) {
  uintptr_t f = 0;
  if (bn)
    f = reinterpret_cast<uintptr_t>(bn->mean) | reinterpret_cast<uintptr_t>(bn->invstd) |
        reinterpret_cast<uintptr_t>(bn->gamma) | reinterpret_cast<uintptr_t>(bn->beta);
  return C % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & (4 * sizeof(E) - 1)) == 0 &&
         (reinterpret_cast<uintptr_t>(idx) & 3) == 0 && (f & 15) == 0;
}

template <class E, bool BN>
static int maxpool_fwd_t(const E* x, int N, int H, int W, int C, int stride, const BnIn& bn, E* y, uint8_t* idx,
                         void* stream) {
  if (!pool_args_ok(N, H, W, C, stride) || !x || !y) return DK_ERR_ARGS;
  if (BN && (!bn.mean || !bn.invstd || !bn.gamma || !bn.beta)) return DK_ERR_ARGS;
  const int OH = H / stride, OW = W / stride;
  const bool vec = pool_vec_ok(C, x, (const E*)y, idx, BN ? &bn : nullptr);
  const long long total = (long long)N * OH * OW * (vec ? C / 4 : C);
  if (cdivll(total, 256) > 0x7fffffffll) return DK_ERR_ARGS;
  const dim3 grid((unsigned)cdivll(total, 256));
#define DK_POOL_FWD(V, S)                                                                                          \
  hipLaunchKernelGGL((maxpool_fwd_kernel<E, V, BN, S>), grid, dim3(256), 0, as_stream(stream), x, H, W, C, stride, \
                     OH, OW, total, bn, y, idx)
  if (vec) {
    if (stride == 2) DK_POOL_FWD(4, 2);
    else if (stride == 3) DK_POOL_FWD(4, 3);
    else DK_POOL_FWD(4, 0);
  } else {
    if (stride == 2) DK_POOL_FWD(1, 2);
    else if (stride == 3) DK_POOL_FWD(1, 3);
    else DK_POOL_FWD(1, 0);
  }
#undef DK_POOL_FWD
  return launch_status();
}

template <class E>
static int maxpool_bwd_t(const E* dy, const uint8_t* idx, int N, int H, int W, int C, int stride, E* dx, void* stream) {
  if (!pool_args_ok(N, H, W, C, stride) || !dy || !idx || !dx) return DK_ERR_ARGS;
  const int OH = H / stride, OW = W / stride;
  const bool vec = pool_vec_ok(C, dy, (const E*)dx, idx, nullptr);
  const long long total = (long long)N * OH * OW * (vec ? C / 4 : C);
  if (cdivll(total, 256) > 0x7fffffffll) return DK_ERR_ARGS;
  const dim3 grid((unsigned)cdivll(total, 256));
#define DK_POOL_BWD(V, S)                                                                                           \
  hipLaunchKernelGGL((maxpool_bwd_kernel<E, V, S>), grid, dim3(256), 0, as_stream(stream), dy, idx, H, W, C, stride, \
                     OH, OW, total, dx)
  if (vec) {
    if (stride == 2) DK_POOL_BWD(4, 2);
    else if (stride == 3) DK_POOL_BWD(4, 3);
    else DK_POOL_BWD(4, 0);
  } else {
    if (stride == 2) DK_POOL_BWD(1, 2);
    else if (stride == 3) DK_POOL_BWD(1, 3);
    else DK_POOL_BWD(1, 0);
  }
#undef DK_POOL_BWD
  return launch_status();
}

}  // namespace dk

using namespace dk;

DK_API int dk_maxpool_fwd_f32(const float* x, int N, int H, int W, int C, int stride, float* y, uint8_t* idx,
                              void* stream) {
  return maxpool_fwd_t<float, false>(x, N, H, W, C, stride, BnIn{nullptr, nullptr, nullptr, nullptr, 0}, y, idx, stream);
}
DK_API int dk_maxpool_fwd_bf16(const uint16_t* x, int N, int H, int W, int C, int stride, uint16_t* y, uint8_t* idx,
                               void* stream) {
  return maxpool_fwd_t<bf16_t, false>(x, N, H, W, C, stride, BnIn{nullptr, nullptr, nullptr, nullptr, 0}, y, idx,
                                      stream);
}
DK_API int dk_maxpool_fwd_bnx_f32(const float* x, int N, int H, int W, int C, int stride, const float* bn_mean,
                                  const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                                  float* y, uint8_t* idx, void* stream) {
  return maxpool_fwd_t<float, true>(x, N, H, W, C, stride, BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, y, idx,
                                    stream);
}
DK_API int dk_maxpool_fwd_bnx_bf16(const uint16_t* x, int N, int H, int W, int C, int stride, const float* bn_mean,
                                   const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                                   uint16_t* y, uint8_t* idx, void* stream) {
  return maxpool_fwd_t<bf16_t, true>(x, N, H, W, C, stride, BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, y,
                                     idx, stream);
}
DK_API int dk_maxpool_bwd_f32(const float* dy, const uint8_t* idx, int N, int H, int W, int C, int stride, float* dx,
                              void* stream) {
  return maxpool_bwd_t<float>(dy, idx, N, H, W, C, stride, dx, stream);
}
DK_API int dk_maxpool_bwd_bf16(const uint16_t* dy, const uint8_t* idx, int N, int H, int W, int C, int stride,
                               uint16_t* dx, void* stream) {
  return maxpool_bwd_t<bf16_t>(dy, idx, N, H, W, C, stride, dx, stream);
}
