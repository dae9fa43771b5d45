// Flatten / unflatten between the NHWC activation layout and the reference's row-major feature order
// (layers/reshape.py: X.reshape((B, C*H*W)) on an NCHW array), gfx950.
//
// Activations are NHWC bytes under a logical NCHW shape, the reference numbers the features of one
// image f = c * HW + p (p = h * W + w), so the flatten is a batched transpose of [HW][C] into [C][HW]
// and its backward the inverse.  The backward kernels are also the forward of an unflatten (2-D -> 4-D)
// and the forward kernels its backward: there are no further kernels.
//
// Pure data movement, so the design is bytes moved with both HBM sides coalesced.  One block of 256
// threads moves a tile of 64 pixels x 64 channels through LDS:
//   * the NHWC side runs along C: 16-byte fp32 / 8-byte bf16 vectors of 4 channels when C % 4 == 0 and
//     the pointers are aligned for them (V = 4), else one element per lane, 64 lanes along C (V = 1: any
//     C, any alignment);
//   * the flat side runs along p: each wave moves 64 consecutive dwords of one channel's row.  The rows
//     are HW elements long and in general not 16-byte aligned (HW = 49), so these stay dword accesses;
//   * the tile is tile[c][p] with a row pitch of 65 dwords.  ds_write_b32 / ds_read_b32 are banked
//     (a / 4) mod 32 over groups of 32 lanes: on the flat side a group's lanes are 32 consecutive p of one
//     c, banks (c + p) mod 32; on the NHWC side a group is 8 channel quads x 4 pixels (V = 4), element e
//     of quad q at pixel p in bank (4 q + e + p) mod 32 with 4 q + p covering 0..31 once, or 32
//     consecutive c of one pixel (V = 1), banks (c + p) mod 32: conflict-free in both directions.
// A bf16 input is widened as it is read (exact); the bf16 backward rounds once, to nearest even, in its
// store.  With BN on load (_bnx) every loaded value goes through bn_in4 / bn_relu_out -- dk_bn_apply_*'s
// arithmetic -- and, for bf16 storage, is rounded to bf16 *before* it is widened: the unfused path
// flattens the stored bf16 BN output, and the two agree bit for bit.
// HW == 1 is the identity on the bytes' order: a plain elementwise pass.
// Every output element is written exactly once (no memset, no atomics); all offsets are 64-bit.
#include "dk_common.h"

namespace dk {

constexpr int kFlatTile = 64;   // pixels and channels per tile
constexpr int kFlatPitch = 65;  // dwords per tile row: odd (1 mod 32), see above

struct FlatTile {
  long long n;
  int c0, p0;
};
__device__ __forceinline__ FlatTile flat_tile(int PT, int CT) {
  long long b = blockIdx.x;
  const int ct = (int)(b % CT);
  b /= CT;
  const int pt = (int)(b % PT);
  return FlatTile{b / PT, ct * kFlatTile, pt * kFlatTile};
}

// The NHWC side of the tile, V = 4: thread t holds channel quad q (the same in every round) and, in
// round i, pixel p.  A group of 32 lanes is 8 quads x 4 pixels; a wave is 4 pixels x 64 channels.
__device__ __forceinline__ int flat_quad(int t) { return (t & 7) + 8 * ((t >> 5) & 1); }
__device__ __forceinline__ int flat_quad_pixel(int t, int i) { return ((t >> 3) & 3) + 4 * ((i * 256 + t) >> 6); }

// x[N][HW][C] (E) -> y[N][C*HW] (fp32), BN: bn(x) [+ ReLU] formed on load, rounded to E's precision
template <class E, int V, bool BN>
__global__ __launch_bounds__(256) void flatten_fwd_kernel(const E* __restrict__ x, int HW, int C, int PT, int CT,
                                                          BnIn bn, float* __restrict__ y) {
  __shared__ float tile[kFlatTile * kFlatPitch];
  const FlatTile T = flat_tile(PT, CT);
  const int t = threadIdx.x;
  const E* xi = x + T.n * HW * C;
  float* yi = y + T.n * C * HW;
  if constexpr (V == 4) {
    const int q = flat_quad(t);
    const int c = T.c0 + 4 * q;
    const bool cok = c < C;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 mu = z4, is = z4, ga = z4, be = z4;
    if constexpr (BN) {
      if (cok) {
        mu = ld4(bn.mean + c);
        is = ld4(bn.invstd + c);
        ga = ld4(bn.gamma + c);
        be = ld4(bn.beta + c);
      }
    }
    f32x4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pp = T.p0 + flat_quad_pixel(t, i);
      v[i] = (cok && pp < HW) ? ld4(xi + (long long)pp * C + c) : z4;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = flat_quad_pixel(t, i);
      if (cok && T.p0 + p < HW) {
        f32x4 o = v[i];
        if constexpr (BN) o = rnd4<E>(bn_in4(o, mu, is, ga, be, bn.relu));
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[(4 * q + e) * kFlatPitch + p] = o[e];
      }
    }
  } else {
    const int cl = t & 63;  // 64 lanes along C; round i takes pixels 4 i .. 4 i + 3, one per wave
    const int c = T.c0 + cl;
    const bool cok = c < C;
    float mu = 0.f, is = 0.f, ga = 0.f, be = 0.f;
    if constexpr (BN) {
      if (cok) {
        mu = bn.mean[c];
        is = bn.invstd[c];
        ga = bn.gamma[c];
        be = bn.beta[c];
      }
    }
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int p = 4 * i + (t >> 6);
      if (cok && T.p0 + p < HW) {
        float o = ld1(xi + (long long)(T.p0 + p) * C + c);
        if constexpr (BN) o = rnd1<E>(bn_relu_out(o, mu, is, ga, be, bn.relu));
        tile[cl * kFlatPitch + p] = o;
      }
    }
  }
  __syncthreads();
  // the flat side: 64 lanes along p, round i takes channels 4 i .. 4 i + 3, one per wave
  const int p = t & 63;
  const bool pok = T.p0 + p < HW;
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int cl = 4 * i + (t >> 6);
    if (pok && T.c0 + cl < C) yi[(long long)(T.c0 + cl) * HW + T.p0 + p] = tile[cl * kFlatPitch + p];
  }
}

// dy[N][C*HW] (fp32) -> dx[N][HW][C] (E; bf16: one round-to-nearest-even in the store)
template <class E, int V>
__global__ __launch_bounds__(256) void flatten_bwd_kernel(const float* __restrict__ dy, int HW, int C, int PT, int CT,
                                                          E* __restrict__ dx) {
  __shared__ float tile[kFlatTile * kFlatPitch];
  const FlatTile T = flat_tile(PT, CT);
  const int t = threadIdx.x;
  const float* dyi = dy + T.n * C * HW;
  E* dxi = dx + T.n * HW * C;
  {
    const int p = t & 63;
    const bool pok = T.p0 + p < HW;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int cl = 4 * i + (t >> 6);
      if (pok && T.c0 + cl < C) tile[cl * kFlatPitch + p] = dyi[(long long)(T.c0 + cl) * HW + T.p0 + p];
    }
  }
  __syncthreads();
  if constexpr (V == 4) {
    const int q = flat_quad(t);
    const int c = T.c0 + 4 * q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = flat_quad_pixel(t, i);
      if (c < C && T.p0 + p < HW) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = tile[(4 * q + e) * kFlatPitch + p];
        st4(dxi + (long long)(T.p0 + p) * C + c, o);
      }
    }
  } else {
    const int cl = t & 63;
    const int c = T.c0 + cl;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int p = 4 * i + (t >> 6);
      if (c < C && T.p0 + p < HW) st1(dxi + (long long)(T.p0 + p) * C + c, tile[cl * kFlatPitch + p]);
    }
  }
}

// HW == 1: [N][1][C] and [N][C] hold the elements in the same order
template <class In, class Out, bool BN>
__global__ __launch_bounds__(256) void flatten_copy_kernel(const In* __restrict__ x, long long total, int C, BnIn bn,
                                                           Out* __restrict__ y) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  float v = ld1(x + t);
  if constexpr (BN) {
    const int c = (int)(t % C);
    v = rnd1<In>(bn_relu_out(v, bn.mean[c], bn.invstd[c], bn.gamma[c], bn.beta[c], bn.relu));
  }
  st1(y + t, v);
}

// blocks of the tiled kernels (0: the sizes are refused)
static inline long long flat_blocks(int N, int HW, int C) {
  if (N < 1 || HW < 1 || C < 1) return 0;
  const long long b = (long long)N * cdiv(HW, kFlatTile) * cdiv(C, kFlatTile);
  return b > 0x7fffffffll ? 0 : b;
}

template <class E, bool BN>
static int flatten_fwd_t(const E* x, int N, int HW, int C, const BnIn& bn, float* y, void* stream) {
  const long long blocks = flat_blocks(N, HW, C);
  if (!blocks || !x || !y) return DK_ERR_ARGS;
  if (BN && (!bn.mean || !bn.invstd || !bn.gamma || !bn.beta)) return DK_ERR_ARGS;
  if (HW == 1) {
    const long long total = (long long)N * C;
    hipLaunchKernelGGL((flatten_copy_kernel<E, float, BN>), dim3((unsigned)cdivll(total, 256)), dim3(256), 0,
                       as_stream(stream), x, total, C, bn, y);
    return launch_status();
  }
  uintptr_t a = reinterpret_cast<uintptr_t>(x) & (4 * sizeof(E) - 1);
  if (BN)
    a |= (reinterpret_cast<uintptr_t>(bn.mean) | reinterpret_cast<uintptr_t>(bn.invstd) |
          reinterpret_cast<uintptr_t>(bn.gamma) | reinterpret_cast<uintptr_t>(bn.beta)) & 15;
  const int PT = cdiv(HW, kFlatTile), CT = cdiv(C, kFlatTile);
  if (C % 4 == 0 && a == 0)
    hipLaunchKernelGGL((flatten_fwd_kernel<E, 4, BN>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, HW,
                       C, PT, CT, bn, y);
  else
    hipLaunchKernelGGL((flatten_fwd_kernel<E, 1, BN>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, HW,
                       C, PT, CT, bn, y);
  return launch_status();
}

template <class E>
static int flatten_bwd_t(const float* dy, int N, int HW, int C, E* dx, void* stream) {
  const long long blocks = flat_blocks(N, HW, C);
  if (!blocks || !dy || !dx) return DK_ERR_ARGS;
  if (HW == 1) {
    const long long total = (long long)N * C;
    hipLaunchKernelGGL((flatten_copy_kernel<float, E, false>), dim3((unsigned)cdivll(total, 256)), dim3(256), 0,
                       as_stream(stream), dy, total, C, BnIn{nullptr, nullptr, nullptr, nullptr, 0}, dx);
    return launch_status();
  }
  const int PT = cdiv(HW, kFlatTile), CT = cdiv(C, kFlatTile);
  if (C % 4 == 0 && (reinterpret_cast<uintptr_t>(dx) & (4 * sizeof(E) - 1)) == 0)
    hipLaunchKernelGGL((flatten_bwd_kernel<E, 4>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), dy, HW, C,
                       PT, CT, dx);
  else
    hipLaunchKernelGGL((flatten_bwd_kernel<E, 1>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), dy, HW, C,
                       PT, CT, dx);
  return launch_status();
}

}  // namespace dk

using namespace dk;

DK_API int dk_flatten_fwd_f32(const float* x, int N, int HW, int C, float* y, void* stream) {
  return flatten_fwd_t<float, false>(x, N, HW, C, BnIn{nullptr, nullptr, nullptr, nullptr, 0}, y, stream);
}
DK_API int dk_flatten_fwd_bf16(const uint16_t* x, int N, int HW, int C, float* y, void* stream) {
  return flatten_fwd_t<bf16_t, false>(x, N, HW, C, BnIn{nullptr, nullptr, nullptr, nullptr, 0}, y, stream);
}
DK_API int dk_flatten_fwd_bnx_f32(const float* x, int N, int HW, int C, const float* bn_mean, const float* bn_invstd,
                                  const float* bn_gamma, const float* bn_beta, int bn_relu, float* y, void* stream) {
  return flatten_fwd_t<float, true>(x, N, HW, C, BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, y, stream);
}
DK_API int dk_flatten_fwd_bnx_bf16(const uint16_t* x, int N, int HW, int C, const float* bn_mean,
                                   const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                                   float* y, void* stream) {
  return flatten_fwd_t<bf16_t, true>(x, N, HW, C, BnIn{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu}, y, stream);
}
DK_API int dk_flatten_bwd_f32(const float* dy, int N, int HW, int C, float* dx, void* stream) {
  return flatten_bwd_t<float>(dy, N, HW, C, dx, stream);
}
DK_API int dk_flatten_bwd_bf16(const float* dy, int N, int HW, int C, uint16_t* dx, void* stream) {
  return flatten_bwd_t<bf16_t>(dy, N, HW, C, dx, stream);
}
