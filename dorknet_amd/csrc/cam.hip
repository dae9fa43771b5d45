// Class activation maps: the reference's returnCAM + show_cam_on_image
// (examples/imagenet_dogs_225_resnet_18_depsep_CAM.py:13-49) for N images x K classes in one launch,
// and the arg-sort that picks the classes (:75), both on the device.
//
//   cam     per (image, class): the h x w dot product of the feature map with one column of the dense
//           weights, cv2.resize (INTER_LINEAR, fp32) to H x W, clip at 0, subtract the minimum, divide by
//           the range, COLORMAP_JET, add the image, divide by the maximum, uint8.  Bit-exact to
//           tests/_cam_ref.py (cam_f32); cv2 is not installed to compare against, so agreement with
//           cv2's own resize and colour map is unpinned.
//   top-k   np.argsort(scores)[::-1][:K] per row: K rounds of an arg-max, equal scores higher index first.
#include "dk_common.h"

// Every fp32 / fp64 operation is rounded on its own, as in the numpy restatement: no contraction.  The
// arithmetic is written out as plain expressions so that this pragma governs all of it (an inline
// function from a header keeps the contraction mode it was compiled under).
#pragma clang fp contract(off)

namespace dk {

constexpr int kCamThreads = 1024;   // 16 waves: one workgroup per (image, class) map
constexpr int kCamWaves = kCamThreads / 64;
constexpr int kCamMaxMap = 1024;    // h * w positions kept in LDS
constexpr int kCamWCap = 4096;      // channels of the weight column staged in LDS; the rest is read in place

// One axis of cv2.resize INTER_LINEAR for fp32 (OpenCV 4.3 imgproc/src/resize.cpp, restated):
//   f = (float)((o + 0.5) * scale - 0.5), s = floor(f), f -= s; s < 0 -> (0, 0); s >= L - 1 -> (L - 1, 0);
// the second tap's index is clamped (its weight is 0 there).  scale = (double)L / O, O >= 1, so
// -0.5 <= f < L and s fits an int.
struct CamAxis {
  int s0, s1;
  float f;
};
__device__ __forceinline__ CamAxis cam_axis(int o, double scale, int L) {
  float f = (float)(((double)o + 0.5) * scale - 0.5);
  const float fl = floorf(f);
  int s = (int)fl;
  f = f - fl;
  if (s < 0) {
    s = 0;
    f = 0.f;
  }
  if (s >= L - 1) {
    s = L - 1;
    f = 0.f;
  }
  CamAxis a;
  a.s0 = s;
  a.s1 = min(s + 1, L - 1);
  a.f = f;
  return a;
}

// The enlarged, clipped map at output pixel (y, x): horizontal pass on both rows, then the vertical one.
__device__ __forceinline__ float cam_value(const float* S, int w, CamAxis ay, CamAxis ax) {
  const float gx = 1.f - ax.f, gy = 1.f - ay.f;
  const float* r0 = S + ay.s0 * w;
  const float* r1 = S + ay.s1 * w;
  const float t0 = r0[ax.s0] * gx + r0[ax.s1] * ax.f;
  const float t1 = r1[ax.s0] * gx + r1[ax.s1] * ax.f;
  const float u = t0 * gy + t1 * ay.f;
  return u > 0.f ? u : 0.f;   // np.maximum(cam, 0) for every finite u
}

// COLORMAP_JET entry i as b | g << 8 | r << 16: round_half_even(255 v) of b = clamp01(min(i + 32, 160 - i) / 64),
// g = clamp01(min(i - 31, 224 - i) / 64), r = b[255 - i] (integers: 255 * num / 64, ties to even).
__device__ __forceinline__ uint32_t jet_level(int num) {
  num = min(max(num, 0), 64) * 255;
  const int q = num >> 6, rem = num & 63;
  return (uint32_t)(q + ((rem > 32 || (rem == 32 && (q & 1))) ? 1 : 0));
}
__device__ __forceinline__ uint32_t jet_entry(int i) {
  const uint32_t b = jet_level(min(i + 32, 160 - i)), g = jet_level(min(i - 31, 224 - i));
  const int j = 255 - i;
  const uint32_t r = jet_level(min(j + 32, 160 - j));
  return b | g << 8 | r << 16;
}

// (uint8)(255 * m), truncating; clamped, and a NaN takes 0, so it can index the table
__device__ __forceinline__ int cam_level(float m) {
  const float r = 255.f * m;
  return r >= 0.f ? (r <= 255.f ? (int)r : 255) : 0;
}

// min and max over the workgroup (order-free); red: 2 * kCamWaves floats of LDS
__device__ __forceinline__ void block_min_max(float& mn, float& mx, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();   // (red may still be read from the previous reduction)
  if ((threadIdx.x & 63) == 0) {
    red[2 * wave] = mn;
    red[2 * wave + 1] = mx;
  }
  __syncthreads();
  mn = red[0];
  mx = red[1];
  for (int i = 1; i < kCamWaves; ++i) {
    mn = fminf(mn, red[2 * i]);
    mx = fmaxf(mx, red[2 * i + 1]);
  }
}

// One workgroup per (n, k).  The h x w map lives in LDS and the enlarged value is recomputed in each of
// the three sweeps over H x W (min / max of the map; max of heat + image; the stores), so nothing
// intermediate goes to HBM.  A lane owns one pixel per step: the image planes are read and the mask is
// written as 256 adjacent bytes per wave, and four neighbouring lanes pack their 12 overlay bytes into
// three dwords (192 adjacent bytes per wave).  The pixel index is offset by `pad` so that those dwords
// are 4-byte aligned; a group cut by either end of the map stores bytes.
template <class T>
__global__ __launch_bounds__(kCamThreads) void cam_kernel(const T* __restrict__ feat, int h, int w, int C,
                                                          const float* __restrict__ weights, int classes,
                                                          const int* __restrict__ class_idx,
                                                          const float* __restrict__ image, int H, int W,
                                                          float shift, float* __restrict__ mask,
                                                          uint8_t* __restrict__ overlay, int K, double scy,
                                                          double scx) {
  __shared__ float S[kCamMaxMap];
  __shared__ float wcol[kCamWCap];
  __shared__ uint32_t jet[256];
  __shared__ float red[2 * kCamWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t map = blockIdx.x;   // n * K + k
  const int n = (int)(map / K);
  // a bad index is clamped: it cannot read outside the weights
  const int cls = min(max(class_idx[map], 0), classes - 1);
  const int hw = h * w, HW = H * W;

  if (tid < 256) jet[tid] = jet_entry(tid);
  for (int c = tid; c < min(C, kCamWCap); c += kCamThreads) wcol[c] = weights[(size_t)c * classes + cls];
  __syncthreads();

  // the dot product: one wave per position, lane j sums channels j, j + 64, ... in ascending order
  // (product rounded, then the sum), then the fixed tree s_j += s_{j + d}, d = 32 ... 1
  const T* fn = feat + (size_t)n * hw * C;
  for (int p = wave; p < hw; p += kCamWaves) {
    const T* fp = fn + (size_t)p * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float wv = c < kCamWCap ? wcol[c] : weights[(size_t)c * classes + cls];
      s = s + wv * ld1(fp + c);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s = s + __shfl_down(s, d, 64);
    if (lane == 0) S[p] = s;
  }
  __syncthreads();

  // overlay bytes of pixel q start at ob + 3 q: groups of four pixels starting at q = -pad (mod 4) are
  // dword aligned
  uint8_t* ob = overlay ? overlay + map * (size_t)HW * 3 : nullptr;
  const int pad = ob ? (int)((4 - ((uintptr_t)ob & 3)) & 3) : 0;
  const int steps = (HW + pad + kCamThreads - 1) / kCamThreads;   // the same for every lane (HW checked on the host)

  // sweep 1: min and max of the clipped, enlarged map
  float mn = INFINITY, mx = -INFINITY;
  for (int it = 0; it < steps; ++it) {
    const int q = it * kCamThreads + tid - pad;
    if (q >= 0 && q < HW) {
      const int y = q / W, x = q - y * W;
      const float v = cam_value(S, w, cam_axis(y, scy, h), cam_axis(x, scx, w));
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
  }
  block_min_max(mn, mx, red);
  const float range = mx - mn;
  const bool scale = range > 0.f;   // the reference's `if np.max(cam) > 0`

  const float* im = image ? image + (size_t)n * 3 * HW : nullptr;
  // sweep 2: the maximum of heat + image over all pixels and channels
  float M = 1.f;
  if (ob) {
    float lo = INFINITY, hi = -INFINITY;
    for (int it = 0; it < steps; ++it) {
      const int q = it * kCamThreads + tid - pad;
      if (q >= 0 && q < HW) {
        const int y = q / W, x = q - y * W;
        const float v = cam_value(S, w, cam_axis(y, scy, h), cam_axis(x, scx, w));
        float m = v - mn;
        if (scale) m = m / range;
        const uint32_t heat = jet[cam_level(m)];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float o = (float)((heat >> (8 * c)) & 255u) + (im[(size_t)c * HW + q] + shift);
          hi = fmaxf(hi, o);
        }
      }
    }
    block_min_max(lo, hi, red);
    M = hi;
  }

  // sweep 3: the stores
  float* mo = mask ? mask + map * (size_t)HW : nullptr;
  for (int it = 0; it < steps; ++it) {
    const int q = it * kCamThreads + tid - pad;
    const bool valid = q >= 0 && q < HW;
    uint32_t px = 0;
    if (valid) {
      const int y = q / W, x = q - y * W;
      const float v = cam_value(S, w, cam_axis(y, scy, h), cam_axis(x, scx, w));
      float m = v - mn;
      if (scale) m = m / range;
      if (mo) mo[q] = m;
      if (ob) {
        const uint32_t heat = jet[cam_level(m)];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float o = (float)((heat >> (8 * c)) & 255u) + (im[(size_t)c * HW + q] + shift);
          // (uint8)(255 * (o / M)), truncating; outside 0 <= image + shift <= 255 clamped (a NaN takes 0)
          px |= (uint32_t)cam_level(o / M) << (8 * c);
        }
      }
    }
    if (ob) {   // uniform over the workgroup: every lane takes part in the ballot and the shuffle
      const unsigned long long ok = __ballot(valid);
      const bool full = ((ok >> (lane & ~3)) & 0xFull) == 0xFull;
      const uint32_t nxt = __shfl_down(px, 1, 64);
      const int i = lane & 3;
      if (full) {
        // pixels p0..p3 of 3 bytes each as dwords p0 | p1 << 24, p1 >> 8 | p2 << 16, p2 >> 16 | p3 << 8
        if (i < 3) *reinterpret_cast<uint32_t*>(ob + (size_t)3 * q + i) = (px >> (8 * i)) | (nxt << (24 - 8 * i));
      } else if (valid) {
        uint8_t* o = ob + (size_t)3 * q;
        o[0] = (uint8_t)(px & 255u);
        o[1] = (uint8_t)((px >> 8) & 255u);
        o[2] = (uint8_t)((px >> 16) & 255u);
      }
    }
  }
}

// np.argsort(row)[::-1][:K]: K rounds of an arg-max over the entries not yet taken; of equal scores the
// higher index wins (a stable ascending sort, reversed).  One workgroup of 256 threads per row.
__device__ __forceinline__ bool topk_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i > bi); }

__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ scores, int classes, int K,
                                                        int* __restrict__ idx_out, float* __restrict__ val_out) {
  __shared__ float rv[4];
  __shared__ int ri[4];
  __shared__ int taken[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = scores + (size_t)blockIdx.x * classes;
  for (int r = 0; r < K; ++r) {
    float bv = -INFINITY;
    int bi = -1;
    for (int i = tid; i < classes; i += 256) {
      bool free_ = true;
      for (int t = 0; t < r; ++t) free_ = free_ && taken[t] != i;
      const float v = row[i];
      if (free_ && topk_better(v, i, bv, bi)) {
        bv = v;
        bi = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (topk_better(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      rv[wave] = bv;
      ri[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < 4; ++k)
        if (topk_better(rv[k], ri[k], bv, bi)) {
          bv = rv[k];
          bi = ri[k];
        }
      bi = max(bi, 0);   // only NaN scores leave no winner; the index stays inside the row
      taken[r] = bi;
      idx_out[(size_t)blockIdx.x * K + r] = bi;
      if (val_out) val_out[(size_t)blockIdx.x * K + r] = row[bi];   // dk_topk_rows_vals_f32: the score itself
    }
    __syncthreads();
  }
}

template <class T>
static int launch_cam(const T* feat, int N, int h, int w, int C, const float* weights, int classes,
                      const int* class_idx, int K, const float* image, int H, int W, float shift, float* mask,
                      uint8_t* overlay, void* stream) {
  if (!feat || !weights || !class_idx || N < 1 || K < 1 || h < 1 || w < 1 || H < 1 || W < 1 || C < 1 || classes < 1)
    return DK_ERR_ARGS;
  if ((long long)h * w > kCamMaxMap) return DK_ERR_ARGS;
  if (!mask && !overlay) return DK_ERR_ARGS;
  if (overlay && !image) return DK_ERR_ARGS;
  // the kernel's 32-bit pixel index (plus the alignment offset and one step of the sweep), one map per block
  if ((long long)H * W > 0x7fffffffLL - 2 * kCamThreads || (long long)N * K > 0x7fffffffLL) return DK_ERR_ARGS;
  hipLaunchKernelGGL(cam_kernel<T>, dim3((unsigned)(N * K)), dim3(kCamThreads), 0, as_stream(stream), feat, h, w, C,
                     weights, classes, class_idx, image, H, W, shift, mask, overlay, K, (double)h / (double)H,
                     (double)w / (double)W);
  return launch_status();
}

}  // namespace dk

using namespace dk;

DK_API int dk_cam_f32(const float* feat, int N, int h, int w, int C, const float* weights, int classes,
                      const int* class_idx, int K, const float* image, int H, int W, float shift, float* mask,
                      uint8_t* overlay, void* stream) {
  return launch_cam<float>(feat, N, h, w, C, weights, classes, class_idx, K, image, H, W, shift, mask, overlay, stream);
}

DK_API int dk_cam_bf16(const uint16_t* feat, int N, int h, int w, int C, const float* weights, int classes,
                       const int* class_idx, int K, const float* image, int H, int W, float shift, float* mask,
                       uint8_t* overlay, void* stream) {
  return launch_cam<bf16_t>(feat, N, h, w, C, weights, classes, class_idx, K, image, H, W, shift, mask, overlay,
                            stream);
}

DK_API int dk_topk_rows_f32(const float* scores, int N, int classes, int K, int* idx_out, void* stream) {
  if (!scores || !idx_out || N < 1 || classes < 1 || K < 1 || K > 16 || K > classes) return DK_ERR_ARGS;
  hipLaunchKernelGGL(topk_rows_kernel, dim3((unsigned)N), dim3(256), 0, as_stream(stream), scores, classes, K, idx_out,
                     (float*)nullptr);
  return launch_status();
}

DK_API int dk_topk_rows_vals_f32(const float* scores, int N, int classes, int K, int* idx_out, float* val_out,
                                 void* stream) {
  if (!scores || !idx_out || !val_out || N < 1 || classes < 1 || K < 1 || K > 16 || K > classes) return DK_ERR_ARGS;
  hipLaunchKernelGGL(topk_rows_kernel, dim3((unsigned)N), dim3(256), 0, as_stream(stream), scores, classes, K, idx_out,
                     val_out);
  return launch_status();
}
