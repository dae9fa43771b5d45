// Evaluation counters: accuracy, top-k, confusion matrix and loss of a batch of
// score rows against integer labels, accumulated into device-resident int64 words so that a validation
// run reads the host side once, at its end (the reference's FeedForwardNetwork.test copies every batch's
// scores to the host, network/feed_forward_network.py:72-80).
//
// Per row b with label y and scores s (definitions pinned by tests/_metrics_ref.py):
//   pred  np.argmax(s): of equal maxima the lowest index (the rule of `test`);
//   rank  #{j : s[j] > s[y]} + #{j > y : s[j] == s[y]}: the position of y in np.argsort(s, kind="stable")[::-1],
//         so rank < k exactly when y is among dk_topk_rows_f32's first k (equal scores: higher index first);
//   nll   -logf(s[y]), the logf of softmax_xent_fwd_kernel (losses.py:23-26 for a one-hot label).
// pred == y and rank == 0 can differ only on a row whose maximum is tied.
//
// Every counter is an integer, the loss included (llrint(nll * 2^32), Q32): integer adds commute, so any
// number of workgroups may add with plain atomics and two runs give the same bits.
#include "dk_common.h"

namespace dk {

constexpr int kClsWaves = 4;                    // one wave per row, four rows per workgroup and pass
constexpr int kClsThreads = 64 * kClsWaves;
constexpr int kClsRegs = 16;                    // columns a lane keeps in registers
constexpr int kClsTile = 64 * kClsRegs;         // 1024 columns: a longer row is read again for the rank
constexpr int kClsMaxBlocks = 2048;
constexpr int kClsRankBins = 16;                // state[5 + r], r < 16; state[21]: rank >= 16

// (value, index) order of the arg-max: the larger value, of equal values the lower index.  A NaN never wins.
__device__ __forceinline__ bool cls_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// Column of register i of a lane within a tile: float4 chunks lane, lane + 64, ... (V4) or scalars
// lane, lane + 64, ...
template <bool V4>
__device__ __forceinline__ int cls_col(int lane, int i) {
  return V4 ? 4 * (lane + 64 * (i >> 2)) + (i & 3) : lane + 64 * i;
}

// The lane's columns of the tile starting at column `base`, all loads issued at once; a column past the
// row's end holds NaN, which wins no maximum and counts in no rank.
template <bool V4>
__device__ __forceinline__ void cls_load(const float* __restrict__ row, int base, int classes, int lane,
                                         float (&v)[kClsRegs]) {
  if constexpr (V4) {
#pragma unroll
    for (int q = 0; q < kClsRegs / 4; ++q) {
      const int c = base + 4 * (lane + 64 * q);   // classes % 4 == 0: a chunk is inside the row or past it
      const f32x4 x = c < classes ? ld4(row + c) : f32x4{NAN, NAN, NAN, NAN};
#pragma unroll
      for (int u = 0; u < 4; ++u) v[4 * q + u] = x[u];
    }
  } else {
#pragma unroll
    for (int i = 0; i < kClsRegs; ++i) {
      const int c = base + lane + 64 * i;
      v[i] = c < classes ? row[c] : NAN;
    }
  }
}

template <bool V4>
__global__ __launch_bounds__(kClsThreads) void classify_accumulate_kernel(
    const float* __restrict__ scores, const int* __restrict__ labels, int N, int classes,
    unsigned long long* __restrict__ state, unsigned long long* __restrict__ confusion, int* __restrict__ pred_out,
    int* __restrict__ rank_out, float* __restrict__ nll_out) {
  __shared__ unsigned long long part[DK_CLASSIFY_STATE_WORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < DK_CLASSIFY_STATE_WORDS) part[threadIdx.x] = 0ull;
  __syncthreads();

  const int tiles = (classes + kClsTile - 1) / kClsTile;
  for (long long b = (long long)blockIdx.x * kClsWaves + wave; b < N; b += (long long)gridDim.x * kClsWaves) {
    const float* row = scores + (size_t)b * classes;
    const int y = labels[b];
    const bool counted = y >= 0 && y < classes;

    // pass 1: the maximum and its lowest index, per lane, then a fixed butterfly (every lane ends with
    // the same pair)
    float v[kClsRegs];
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int t = 0; t < tiles; ++t) {
      cls_load<V4>(row, t * kClsTile, classes, lane, v);
#pragma unroll
      for (int i = 0; i < kClsRegs; ++i) {
        const int c = t * kClsTile + cls_col<V4>(lane, i);
        if (cls_better(v[i], c, bv, bi)) {
          bv = v[i];
          bi = c;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (cls_better(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    const int pred = bi < classes ? bi : 0;   // only a row of NaNs leaves no winner; the index stays inside the row

    // pass 2: the rank of the label's score, over the registers (one tile) or the row read again
    int rank = -1;
    float nll = 0.f;
    if (counted) {
      const float sy = row[y];
      int cnt = 0;
      for (int t = 0; t < tiles; ++t) {
        if (tiles > 1) cls_load<V4>(row, t * kClsTile, classes, lane, v);
#pragma unroll
        for (int i = 0; i < kClsRegs; ++i) {
          const int c = t * kClsTile + cls_col<V4>(lane, i);
          cnt += (v[i] > sy || (v[i] == sy && c > y)) ? 1 : 0;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      rank = cnt;
      nll = -logf(sy);
    }

    if (lane == 0) {
      if (pred_out) pred_out[b] = pred;
      if (rank_out) rank_out[b] = rank;
      if (nll_out) nll_out[b] = nll;
      if (counted) {
        atomicAdd(&part[0], 1ull);
        if (pred == y) atomicAdd(&part[2], 1ull);
        if (isfinite(nll))
          atomicAdd(&part[4], (unsigned long long)llrint((double)nll * 4294967296.0));
        else
          atomicAdd(&part[3], 1ull);
        atomicAdd(&part[5 + (rank < kClsRankBins ? rank : kClsRankBins)], 1ull);
        if (confusion) atomicAdd(confusion + (size_t)y * classes + pred, 1ull);
      } else {
        atomicAdd(&part[1], 1ull);
      }
    }
  }

  // the workgroup's partial: one atomic per word that it touched
  __syncthreads();
  if (threadIdx.x < DK_CLASSIFY_STATE_WORDS) {
    const unsigned long long p = part[threadIdx.x];
    if (p) atomicAdd(state + threadIdx.x, p);
  }
}

}  // namespace dk

using namespace dk;

DK_API int dk_classify_accumulate_f32(const float* scores, const int* labels, int N, int classes, long long* state,
                                      long long* confusion, int* pred_out, int* rank_out, float* nll_out,
                                      void* stream) {
  if (!scores || !labels || !state || N < 1 || classes < 2) return DK_ERR_ARGS;
  if (classes > 0x7fffffff - kClsTile) return DK_ERR_ARGS;   // the kernel's 32-bit column index, one tile past the end
  const long long groups = cdivll(N, kClsWaves);
  const int blocks = (int)(groups < kClsMaxBlocks ? groups : kClsMaxBlocks);
  unsigned long long* st = reinterpret_cast<unsigned long long*>(state);
  unsigned long long* cf = reinterpret_cast<unsigned long long*>(confusion);
  const bool v4 = classes % 4 == 0 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0;
  if (v4)
    hipLaunchKernelGGL(classify_accumulate_kernel<true>, dim3((unsigned)blocks), dim3(kClsThreads), 0,
                       as_stream(stream), scores, labels, N, classes, st, cf, pred_out, rank_out, nll_out);
  else
    hipLaunchKernelGGL(classify_accumulate_kernel<false>, dim3((unsigned)blocks), dim3(kClsThreads), 0,
                       as_stream(stream), scores, labels, N, classes, st, cf, pred_out, rank_out, nll_out);
  return launch_status();
}
