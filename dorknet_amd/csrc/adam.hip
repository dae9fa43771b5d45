// Adam / AdamW (decoupled decay) as one multi-tensor launch, and clipping by the global gradient
// norm, gfx950.  No optimiser of the reference: an extension (optimisers/Adam.py, optimisers/clip.py;
// DESIGN.md section 21).  The update is torch.optim.Adam / AdamW (non-amsgrad) written as single fp32
// operations; the host forms the scalars in double and rounds each to fp32 once:
//   omb1 = 1 - beta1;  omb2 = 1 - beta2;  neg_step = -(lr / (1 - beta1^t));  sbc2 = sqrt(1 - beta2^t);
//   keep = 1 - lr * weight_decay
// Per element, each operation one correctly rounded fp32 operation, in this order:
//   g' = s * g                      (only with a clip scale s = grad_scale[0])
//   w  = keep * w                   (only for rows with flag bit 0, and keep != 1)
//   m  = beta1 * m + omb1 * g'
//   v  = beta2 * v + omb2 * (g' * g')
//   den = sqrt(v) / sbc2 + eps
//   w  = w + neg_step * (m / den)
// g is read only; m, v and w are written once each.  No contraction (the operations are compiled
// with contraction off), sqrtf and the full division sequence, denormals kept.
//
// The norm: stage 1 writes one fp64 sum of squares per 2048-element chunk, stage 2 (one block) adds
// them in a fixed order: bit-identical from run to run, and across ranks holding the same gradients.
#include "dk_common.h"

namespace dk {

struct AdamEntry {  // 56 bytes
  float* w;
  const float* g;
  float* m;
  float* v;
  long long n;
  long long block0;  // first block index owned by this tensor
  long long flags;   // bit 0: apply keep (decoupled weight decay)
};

struct GradEntry {  // 24 bytes
  float* g;
  long long n;
  long long block0;
};

constexpr int kOwnerLds = 1024;
constexpr int kGradChunk = 2048;  // elements per block of the norm and scale kernels

// The table entry owning this block (the last one with block0 <= blockIdx.x), by binary search over
// the block0 column held in LDS, or by a linear scan of the global table past kOwnerLds entries.
// Called by all 256 threads of the block (it holds barriers).
template <class Entry>
__device__ __forceinline__ Entry owner_entry(const Entry* __restrict__ tab, int ntens) {
  __shared__ long long b0s[kOwnerLds];
  __shared__ int owner;
  const long long b = blockIdx.x;
  int t = 0;
  if (ntens <= kOwnerLds) {
    for (int i = threadIdx.x; i < ntens; i += blockDim.x) b0s[i] = tab[i].block0;
    __syncthreads();
    if (threadIdx.x == 0) {
      int lo = 0, hi = ntens - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (b0s[mid] <= b) lo = mid; else hi = mid - 1;
      }
      owner = lo;
    }
    __syncthreads();
    t = owner;
  } else {
    while (t + 1 < ntens && tab[t + 1].block0 <= b) ++t;
  }
  return tab[t];
}

// One fp32 operation, one rounding: compiled with contraction off, so never fused with a neighbour
// (elementwise.hip's helpers of the same names).
__device__ __forceinline__ float mul_1r(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_1r(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamEntry* __restrict__ tab, int ntens, float beta1,
                                                         float omb1, float beta2, float omb2, float neg_step,
                                                         float sbc2, float eps, float keep,
                                                         const float* __restrict__ grad_scale) {
  const AdamEntry e = owner_entry(tab, ntens);
  const long long i = ((long long)blockIdx.x - e.block0) * 256 + threadIdx.x;
  if (i >= e.n) return;
  float g = e.g[i];
  if (grad_scale) g = mul_1r(grad_scale[0], g);
  float w = e.w[i];
  if ((e.flags & 1) && keep != 1.0f) w = mul_1r(keep, w);
  const float m = add_1r(mul_1r(beta1, e.m[i]), mul_1r(omb1, g));
  const float v = add_1r(mul_1r(beta2, e.v[i]), mul_1r(omb2, mul_1r(g, g)));
  const float den = add_1r(__fdiv_rn(sqrtf(v), sbc2), eps);
  e.w[i] = add_1r(w, mul_1r(neg_step, __fdiv_rn(m, den)));
  e.m[i] = m;
  e.v[i] = v;
}

// Sum of 256 doubles in a fixed tree; the result is in red[0] (thread 0 reads it).
__device__ __forceinline__ void block_sum(double* red, double s) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
}

// Stage 1: part[b] = sum of g^2 over block b's chunk, in fp64.
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const GradEntry* __restrict__ tab, int ntens,
                                                                double* __restrict__ part) {
  __shared__ double red[256];
  const GradEntry e = owner_entry(tab, ntens);
  const long long i0 = ((long long)blockIdx.x - e.block0) * kGradChunk;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kGradChunk / 256; ++k) {
    const long long i = i0 + k * 256 + threadIdx.x;
    if (i < e.n) {
      const double x = e.g[i];
      s += x * x;
    }
  }
  block_sum(red, s);
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// Stage 2 (one block): out[0] = (float)sqrt(sum_b part[b]), out[1] = min(1, max_norm / (out[0] + 1e-6f))
// (torch's clip_grad_norm_), or 1 when max_norm is not a positive finite number (measure only).
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ part, long long nparts,
                                                              float max_norm, float* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (long long i = threadIdx.x; i < nparts; i += 256) s += part[i];
  block_sum(red, s);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    float scale = 1.0f;
    if (max_norm > 0.0f && max_norm <= 3.402823466e38f) {
      const float q = __fdiv_rn(max_norm, add_1r(norm, 1e-6f));
      scale = q < 1.0f ? q : 1.0f;
    }
    out[0] = norm;
    out[1] = scale;
  }
}

// g = scale[0] * g in place; a scale of exactly 1 writes nothing.
__global__ __launch_bounds__(256) void grad_scale_kernel(const GradEntry* __restrict__ tab, int ntens,
                                                         const float* __restrict__ scale) {
  const float s = scale[0];
  if (s == 1.0f) return;
  const GradEntry e = owner_entry(tab, ntens);
  const long long i0 = ((long long)blockIdx.x - e.block0) * kGradChunk;
#pragma unroll
  for (int k = 0; k < kGradChunk / 256; ++k) {
    const long long i = i0 + k * 256 + threadIdx.x;
    if (i < e.n) e.g[i] = mul_1r(s, e.g[i]);
  }
}

static bool table_args_ok(const void* table, int ntens, long long total_blocks) {
  return ntens >= 0 && total_blocks >= 0 && total_blocks <= 0x7fffffffll && (table || ntens == 0);
}

DK_API int dk_adam_multi_f32(const void* table, int ntens, long long total_blocks, float beta1, float omb1,
                             float beta2, float omb2, float neg_step, float sbc2, float eps, float keep,
                             const float* grad_scale, void* stream) {
  if (!table_args_ok(table, ntens, total_blocks)) return DK_ERR_ARGS;
  if (ntens == 0 || total_blocks == 0) return 0;
  hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(stream),
                     static_cast<const AdamEntry*>(table), ntens, beta1, omb1, beta2, omb2, neg_step, sbc2, eps, keep,
                     grad_scale);
  return launch_status();
}

DK_API size_t dk_grad_norm_workspace_bytes(long long total_blocks) {
  return total_blocks > 0 ? (size_t)total_blocks * sizeof(double) : 0;
}

DK_API int dk_grad_norm_multi_f32(const void* table, int ntens, long long total_blocks, float max_norm, float* out,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (!table_args_ok(table, ntens, total_blocks) || !out) return DK_ERR_ARGS;
  if (ntens == 0) total_blocks = 0;
  if (total_blocks > 0 && (!ws || ws_bytes < dk_grad_norm_workspace_bytes(total_blocks))) return DK_ERR_WORKSPACE;
  if (total_blocks > 0) {
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(stream),
                       static_cast<const GradEntry*>(table), ntens, static_cast<double*>(ws));
    const int rc = launch_status();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, as_stream(stream),
                     static_cast<const double*>(ws), total_blocks, max_norm, out);
  return launch_status();
}

DK_API int dk_grad_scale_multi_f32(const void* table, int ntens, long long total_blocks, const float* scale,
                                   void* stream) {
  if (!table_args_ok(table, ntens, total_blocks) || !scale) return DK_ERR_ARGS;
  if (ntens == 0 || total_blocks == 0) return 0;
  hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(stream),
                     static_cast<const GradEntry*>(table), ntens, scale);
  return launch_status();
}

}  // namespace dk
