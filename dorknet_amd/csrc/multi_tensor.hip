// Every kernel that walks a table of tensors in one launch, gfx950: the optimiser updates (SGD, SGD
// momentum, RMSProp, Adam / AdamW, LARS), the global gradient norm with its scale, the per-tensor norms
// and trust ratios of LARS, and the l2 loss term of a whole network.  The host builds the tables in dorknet_amd/_table.py; the row layouts are part of the
// ABI (include/dorknet_hip.h).  DESIGN.md sections 12, 21 and 22.
//
// A table row is {pointers..., n, first_block, extra words...}; block b of the launch belongs to the
// last row with first_block <= b (owner_index / owner_entry) and works on one chunk of that tensor:
// 256 elements in the updates, 2048 in the reductions, the scale and all three LARS kernels.
//
// The updates are written as single fp32 operations, each rounded once and never fused (mul_1r /
// add_1r, sqrtf, __fdiv_rn), denormals kept, so they are bit-identical to their numpy twins.  The
// reductions write one fp64 partial per block and add the partials in one block, both in a fixed
// order: bit-identical from run to run, and across ranks holding the same data.
#include "dk_common.h"

namespace dk {

// state: SGD momentum's velocity, RMSProp's squared-gradient cache, unused (null) for plain SGD
struct SgdEntry {  // 40 bytes
  float* w;
  const float* g;
  float* v;
  long long n;
  long long block0;  // first block index owned by this tensor
};

struct AdamEntry {  // 56 bytes
  float* w;
  const float* g;
  float* m;
  float* v;
  long long n;
  long long block0;
  long long flags;  // bit 0: apply keep (decoupled weight decay)
};

struct LarsEntry {  // 48 bytes
  float* w;
  const float* g;
  float* v;  // the velocity
  long long n;
  long long block0;
  long long flags;  // bit 0: adapt (scale the step by the tensor's trust ratio, add weight_decay * w)
};

struct GradEntry {  // 24 bytes
  float* g;
  long long n;
  long long block0;
};

struct L2Entry {  // 32 bytes
  const float* w;
  long long n;
  long long block0;
  float strength;
  float pad_;
};

constexpr int kOwnerLds = 1024;
constexpr int kChunk = 2048;  // elements per block of the norm, scale and l2 kernels

// The index of the table entry owning this block (the last one with block0 <= blockIdx.x): the block0
// column is loaded into LDS in parallel (one load latency) and searched there by bisection; a linear
// scan of the global table (~100 dependent loads for the last blocks of a network's table) past
// kOwnerLds entries.  Called by all 256 threads of the block (it holds barriers).
template <class Entry>
__device__ __forceinline__ int owner_index(const Entry* __restrict__ tab, int ntens) {
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
  return t;
}

// The owning entry itself.
template <class Entry>
__device__ __forceinline__ Entry owner_entry(const Entry* __restrict__ tab, int ntens) {
  return tab[owner_index(tab, ntens)];
}

// One fp32 operation, one rounding.  __fmul_rn / __fadd_rn are plain * and + compiled under the
// default contraction mode, and once inlined a product and the sum it feeds may still fuse: plain
// SGD's w + (-lr) * g came out as one v_fma_f32.  An operation compiled with contraction off
// carries no contract flag and is never fused.
__device__ __forceinline__ float mul_1r(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_1r(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// ---- the optimiser updates: one block per 256 elements ---------------------------------------------

// Plain SGD:  d = (-lr) * g;  w += d      (SGD.py:20-24)
__global__ __launch_bounds__(256) void sgd_multi_kernel(const SgdEntry* __restrict__ tab, int ntens, float lr) {
  const SgdEntry e = owner_entry(tab, ntens);
  const long long i = ((long long)blockIdx.x - e.block0) * 256 + threadIdx.x;
  if (i >= e.n) return;
  e.w[i] = add_1r(e.w[i], mul_1r(-lr, e.g[i]));
}

// SGD momentum:  d = (-lr) * g + mom * v;  w += d;  v = d      (SGDMomentum.py:33-39, same op order)
// with g = gscale * g first unless gscale is exactly 1.
__global__ __launch_bounds__(256) void sgd_momentum_multi_kernel(const SgdEntry* __restrict__ tab, int ntens,
                                                                 float lr, float mom, float gscale) {
  const SgdEntry e = owner_entry(tab, ntens);
  const long long i = ((long long)blockIdx.x - e.block0) * 256 + threadIdx.x;
  if (i >= e.n) return;
  const float g = gscale == 1.0f ? e.g[i] : mul_1r(gscale, e.g[i]);
  const float d = add_1r(mul_1r(-lr, g), mul_1r(mom, e.v[i]));
  e.w[i] = add_1r(e.w[i], d);
  e.v[i] = d;
}

// RMSProp:  c = decay * c + (1 - decay) * (g * g);  d = ((-lr) * g) / sqrt(c + eps);  w += d
// (RMSProp.py:28-36, same op order).  sqrtf is v_sqrt_f32 plus its residual correction (__fsqrt_rn
// is the bare 1-ulp instruction); __fdiv_rn is the full division sequence.
__global__ __launch_bounds__(256) void rmsprop_multi_kernel(const SgdEntry* __restrict__ tab, int ntens, float lr,
                                                            float decay, float one_minus_decay, float eps) {
  const SgdEntry e = owner_entry(tab, ntens);
  const long long i = ((long long)blockIdx.x - e.block0) * 256 + threadIdx.x;
  if (i >= e.n) return;
  const float g = e.g[i];
  const float c = add_1r(mul_1r(decay, e.v[i]), mul_1r(one_minus_decay, mul_1r(g, g)));
  const float d = __fdiv_rn(mul_1r(-lr, g), sqrtf(add_1r(c, eps)));
  e.w[i] = add_1r(e.w[i], d);
  e.v[i] = c;
}

// Adam / AdamW (decoupled decay): torch.optim.Adam / AdamW, non-amsgrad (no optimiser of the
// reference; optimisers/Adam.py).  The host forms the scalars in double and rounds each to fp32 once:
//   omb1 = 1 - beta1;  omb2 = 1 - beta2;  neg_step = -(lr / (1 - beta1^t));  sbc2 = sqrt(1 - beta2^t);
//   keep = 1 - lr * weight_decay
// Per element, in this order:
//   g' = s * g                      (only with a clip scale s = grad_scale[0])
//   w  = keep * w                   (only for rows with flag bit 0, and keep != 1)
//   m  = beta1 * m + omb1 * g'
//   v  = beta2 * v + omb2 * (g' * g')
//   den = sqrt(v) / sbc2 + eps
//   w  = w + neg_step * (m / den)
// g is read only; m, v and w are written once each.
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

// ---- the reductions and the scale: one block per 2048 elements -------------------------------------

// The fp64 sum of x^2 over this block's chunk of e's tensor p, left in red[0] (thread 0 reads it).
template <class Entry>
__device__ __forceinline__ void chunk_sum_squares(const Entry& e, const float* __restrict__ p, double* red) {
  const long long i0 = ((long long)blockIdx.x - e.block0) * kChunk;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kChunk / 256; ++k) {
    const long long i = i0 + k * 256 + threadIdx.x;
    if (i < e.n) {
      const double x = p[i];
      s += x * x;
    }
  }
  block_sum(red, s);
}

// The fixed-order sum of part[0 .. nparts) in one block, left in red[0].
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, long long nparts, double* red) {
  double s = 0.0;
  for (long long i = threadIdx.x; i < nparts; i += 256) s += part[i];
  block_sum(red, s);
}

// Gradient norm, stage 1: part[b] = sum of g^2 over block b's chunk.
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const GradEntry* __restrict__ tab, int ntens,
                                                                double* __restrict__ part) {
  __shared__ double red[256];
  const GradEntry e = owner_entry(tab, ntens);
  chunk_sum_squares(e, e.g, red);
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// Stage 2 (one block): out[0] = (float)sqrt(sum_b part[b]), out[1] = min(1, max_norm / (out[0] + 1e-6f))
// (torch's clip_grad_norm_), or 1 when max_norm is not a positive finite number (measure only).
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ part, long long nparts,
                                                              float max_norm, float* __restrict__ out) {
  __shared__ double red[256];
  sum_partials(part, nparts, red);
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
  const long long i0 = ((long long)blockIdx.x - e.block0) * kChunk;
#pragma unroll
  for (int k = 0; k < kChunk / 256; ++k) {
    const long long i = i0 + k * 256 + threadIdx.x;
    if (i < e.n) e.g[i] = mul_1r(s, e.g[i]);
  }
}

// l2 loss term, stage 1: part[b] = 0.5 * strength_t * sum(w^2) over block b's chunk of tensor t.
__global__ __launch_bounds__(256) void l2_multi_partial_kernel(const L2Entry* __restrict__ tab, int ntens,
                                                               double* __restrict__ part) {
  __shared__ double red[256];
  const L2Entry e = owner_entry(tab, ntens);
  chunk_sum_squares(e, e.w, red);
  if (threadIdx.x == 0) part[blockIdx.x] = 0.5 * (double)e.strength * red[0];
}

// Stage 2 (one block): out[0] = (add_to ? add_to[0] : 0) + sum_b part[b].
__global__ __launch_bounds__(256) void l2_multi_final_kernel(const double* __restrict__ part, long long nparts,
                                                             const float* __restrict__ add_to,
                                                             float* __restrict__ out) {
  __shared__ double red[256];
  sum_partials(part, nparts, red);
  if (threadIdx.x == 0) out[0] = (float)((add_to ? (double)add_to[0] : 0.0) + red[0]);
}

// ---- LARS: per-tensor norms, trust ratios and the update, one block per 2048 elements -------------
// (You, Gitman, Ginsburg 2017; optimisers/LARS.py.)  One table of LarsEntry rows drives all three.

// Launch 1: part[2b] = sum of w^2, part[2b + 1] = sum of g^2 over block b's chunk, in fp64.
__global__ __launch_bounds__(256) void lars_partial_kernel(const LarsEntry* __restrict__ tab, int ntens,
                                                           double* __restrict__ part) {
  __shared__ double red[2][256];
  const LarsEntry e = owner_entry(tab, ntens);
  chunk_sum_squares(e, e.w, red[0]);
  chunk_sum_squares(e, e.g, red[1]);
  if (threadIdx.x == 0) {
    part[2 * (long long)blockIdx.x] = red[0][0];
    part[2 * (long long)blockIdx.x + 1] = red[1][0];
  }
}

// Launch 2, one block per tensor t: the fixed-order sums of the tensor's own partials (blocks
// block0_t .. block0_{t+1}, the last row ending at total_blocks), then
//   wn = (float)sqrt(sum w^2);  gn = (float)sqrt(sum g^2)
//   ratio = (trust * wn) / ((gn + wd * wn) + eps)   for an adapted row with wn > 0 and gn > 0, else 1
// and stats[4t .. 4t+3] = {wn, gn, ratio, 0}.  A non-finite norm is not special-cased.
__global__ __launch_bounds__(256) void lars_final_kernel(const LarsEntry* __restrict__ tab, int ntens,
                                                         long long total_blocks, const double* __restrict__ part,
                                                         float trust, float wd, float eps,
                                                         float* __restrict__ stats) {
  __shared__ double red[2][256];
  const int t = blockIdx.x;
  const long long first = tab[t].block0;
  const long long last = t + 1 < ntens ? tab[t + 1].block0 : total_blocks;
  double sw = 0.0, sg = 0.0;
  for (long long b = first + threadIdx.x; b < last; b += 256) {
    sw += part[2 * b];
    sg += part[2 * b + 1];
  }
  block_sum(red[0], sw);
  block_sum(red[1], sg);
  if (threadIdx.x == 0) {
    const float wn = (float)sqrt(red[0][0]);
    const float gn = (float)sqrt(red[1][0]);
    float ratio = 1.0f;
    if ((tab[t].flags & 1) && wn > 0.0f && gn > 0.0f)
      ratio = __fdiv_rn(mul_1r(trust, wn), add_1r(add_1r(gn, mul_1r(wd, wn)), eps));
    float* out = stats + 4 * (long long)t;
    out[0] = wn;
    out[1] = gn;
    out[2] = ratio;
    out[3] = 0.0f;
  }
}

// Launch 3:  g' = g + wd * w (adapted rows, wd != 0);  step = (-lr) * ratio_t;
//            d = step * g' + mom * v;  w += d;  v = d
// SGD momentum's form and op order (SGDMomentum.py:33-39): a row that is not adapted has ratio 1, so
// step is exactly -lr and its update is sgd_momentum_multi_kernel's bit for bit.  g and stats are
// read only; w and v are written once each.
__global__ __launch_bounds__(256) void lars_update_kernel(const LarsEntry* __restrict__ tab, int ntens, float lr,
                                                          float mom, float wd, const float* __restrict__ stats) {
  const int t = owner_index(tab, ntens);
  const LarsEntry e = tab[t];
  const float step = mul_1r(-lr, stats[4 * (long long)t + 2]);
  const bool decay = (e.flags & 1) && wd != 0.0f;
  const long long i0 = ((long long)blockIdx.x - e.block0) * kChunk;
#pragma unroll
  for (int k = 0; k < kChunk / 256; ++k) {
    const long long i = i0 + k * 256 + threadIdx.x;
    if (i < e.n) {
      const float w = e.w[i];
      float g = e.g[i];
      if (decay) g = add_1r(g, mul_1r(wd, w));
      const float d = add_1r(mul_1r(step, g), mul_1r(mom, e.v[i]));
      e.w[i] = add_1r(w, d);
      e.v[i] = d;
    }
  }
}

// ---- the C entries ---------------------------------------------------------------------------------
// table: device array of ntens rows; total_blocks = the sum over the tensors of ceil(n / chunk), the
// first_block of a virtual row ntens.  It is the grid, so it must fit one.

static bool table_args_ok(const void* table, int ntens, long long total_blocks) {
  return ntens >= 0 && total_blocks >= 0 && total_blocks <= 0x7fffffffll && (table || ntens == 0);
}

template <class Entry, class... P, class... A>
static int launch_update(void (*kernel)(const Entry*, int, P...), const void* table, int ntens,
                         long long total_blocks, void* stream, A... args) {
  if (!table_args_ok(table, ntens, total_blocks)) return DK_ERR_ARGS;
  if (ntens == 0 || total_blocks == 0) return 0;
  hipLaunchKernelGGL(kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(stream),
                     static_cast<const Entry*>(table), ntens, args...);
  return launch_status();
}

DK_API int dk_sgd_multi_f32(const void* table, int ntens, long long total_blocks, float lr, void* stream) {
  return launch_update(sgd_multi_kernel, table, ntens, total_blocks, stream, lr);
}

DK_API int dk_sgd_momentum_multi_f32(const void* table, int ntens, long long total_blocks, float lr, float momentum,
                                     float grad_scale, void* stream) {
  return launch_update(sgd_momentum_multi_kernel, table, ntens, total_blocks, stream, lr, momentum, grad_scale);
}

DK_API int dk_rmsprop_multi_f32(const void* table, int ntens, long long total_blocks, float lr, float decay,
                                float one_minus_decay, float eps, void* stream) {
  return launch_update(rmsprop_multi_kernel, table, ntens, total_blocks, stream, lr, decay, one_minus_decay, eps);
}

DK_API int dk_adam_multi_f32(const void* table, int ntens, long long total_blocks, float beta1, float omb1,
                             float beta2, float omb2, float neg_step, float sbc2, float eps, float keep,
                             const float* grad_scale, void* stream) {
  return launch_update(adam_multi_kernel, table, ntens, total_blocks, stream, beta1, omb1, beta2, omb2, neg_step,
                       sbc2, eps, keep, grad_scale);
}

DK_API int dk_grad_scale_multi_f32(const void* table, int ntens, long long total_blocks, const float* scale,
                                   void* stream) {
  if (!scale) return DK_ERR_ARGS;
  return launch_update(grad_scale_kernel, table, ntens, total_blocks, stream, scale);
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

// LARS: launches 1 and 2 (the per-tensor norms and trust ratios), then launch 3 (the update).
DK_API size_t dk_lars_workspace_bytes(long long total_blocks) {
  return total_blocks > 0 ? (size_t)total_blocks * 2 * sizeof(double) : 0;
}

DK_API int dk_lars_norms_multi_f32(const void* table, int ntens, long long total_blocks, float trust,
                                   float weight_decay, float eps, float* stats, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (!table_args_ok(table, ntens, total_blocks) || !stats) return DK_ERR_ARGS;
  if (ntens == 0) return 0;
  if (total_blocks > 0 && (!ws || ws_bytes < dk_lars_workspace_bytes(total_blocks))) return DK_ERR_WORKSPACE;
  const LarsEntry* tab = static_cast<const LarsEntry*>(table);
  if (total_blocks > 0) {
    hipLaunchKernelGGL(lars_partial_kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(stream), tab,
                       ntens, static_cast<double*>(ws));
    const int rc = launch_status();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(lars_final_kernel, dim3((unsigned)ntens), dim3(256), 0, as_stream(stream), tab, ntens,
                     total_blocks, static_cast<const double*>(ws), trust, weight_decay, eps, stats);
  return launch_status();
}

DK_API int dk_lars_multi_f32(const void* table, int ntens, long long total_blocks, float lr, float momentum,
                             float weight_decay, const float* stats, void* stream) {
  if (!stats) return DK_ERR_ARGS;
  return launch_update(lars_update_kernel, table, ntens, total_blocks, stream, lr, momentum, weight_decay, stats);
}

// All l2 loss terms of a network in two launches:
// out[0] = add_to[0] (may be null) + sum_t 0.5 * strength_t * sum(w_t^2).
DK_API size_t dk_l2_multi_workspace_bytes(long long total_blocks) { return (size_t)total_blocks * sizeof(double); }

DK_API int dk_l2_loss_multi_f32(const void* table, int ntens, long long total_blocks, const float* add_to,
                                float* out, void* ws, size_t ws_bytes, void* stream) {
  if (ntens <= 0 || total_blocks <= 0) return DK_ERR_ARGS;  // an empty table is refused here, not skipped
  if (ws_bytes < dk_l2_multi_workspace_bytes(total_blocks)) return DK_ERR_WORKSPACE;
  if (!table_args_ok(table, ntens, total_blocks)) return DK_ERR_ARGS;
  hipLaunchKernelGGL(l2_multi_partial_kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(stream),
                     static_cast<const L2Entry*>(table), ntens, static_cast<double*>(ws));
  const int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(l2_multi_final_kernel, dim3(1), dim3(256), 0, as_stream(stream), static_cast<const double*>(ws),
                     total_blocks, add_to, out);
  return launch_status();
}

}  // namespace dk
