// Host launch layer shared by the pointwise kernel files (pw_stream.hip, pw_stream_bf16.hip,
// pw_deep.hip, pw_deep_bf16.hip) and the entry files that choose between them: the occupancy query,
// the two persistent-grid rules, the table of one kernel family's instantiations and the path choice.
//
// A family is one __global__ template at one channel shape; its forms differ in boolean flags
// only.  The family's grid is sized from the smallest occupancy among its counted forms, and a
// launcher picks a form by index and launches once.  The partial rows a caller allocates
// (PwPlan::rows, dk_common.h) are the rows the launch writes: both read the same plan.
#pragma once
#include "dk_common.h"

namespace dk {

// Resident blocks per CU: the smallest over fs (a failed query or a result below 1 counts as 1).
inline int min_occupancy(const void* const* fs, int n, int threads) {
  int o = 1 << 20;
  for (int i = 0; i < n; ++i) {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, fs[i], threads, 0) != hipSuccess || v < 1) v = 1;
    o = v < o ? v : o;
  }
  return o;
}


// Blocks of a streaming grid (WAVES waves per block, each walking TR-pixel tiles): every resident
// slot once, at most one block per WAVES tiles.  A function of its arguments only, so the row count
// a caller allocates for is the count the launch uses and the summation order is reproducible.
inline int pw_stream_grid(int M, int TR, int WAVES, int occ) {
  const int ntiles = (M + TR - 1) / TR;
  const int want = (ntiles + WAVES - 1) / WAVES;
  const int slots = occ * kNumCUs;
  return want < slots ? (want > 0 ? want : 1) : slots;
}

// Row-tile walkers per column group of a deep grid (N output columns in groups of NB, tr-pixel
// tiles): every resident slot once (all blocks of a CU run at the same time, so each CU gets the
// same number of blocks and each block within one tile of the same share), at most one walker per
// tile; a multiple of the 8 XCDs when that costs no extra tile per walker, so that walker x of every
// column group runs on one XCD (block id x + gx * y) and the groups of a row tile share that XCD's
// L2 copy of its pixels.  N < NB (the C = 64 fused backward) is one column group.
inline int pw_deep_grid(int M, int N, int NB, int tr, int occ) {
  const int ntiles = (M + tr - 1) / tr;
  const int groups = N < NB ? 1 : N / NB;
  int slots = occ * kNumCUs / groups;
  if (slots < 1) slots = 1;
  int gx = ntiles < slots ? ntiles : slots;
  const int g8 = gx / 8 * 8;
  if (g8 >= 8 && (ntiles + g8 - 1) / g8 == (ntiles + gx - 1) / gx) gx = g8;
  return gx;
}

// The forms of one family, indexed by their flags (DK_PW_Fn: the first flag is the index's highest
// bit).  counted: bit i set = form i counts towards the family's occupancy; every launched form that
// is left out says why where the table is built.  occ is filled by pw_table(), once, as the
// function-local static holding the table is initialised (thread-safe).
template <int NF, class... A>
struct PwKernelTable {
  void (*fn[NF])(A...);
  int threads;  // block size
  uint32_t counted;
  int occ;
  void launch(int i, dim3 grid, hipStream_t st, A... a) const {
    hipLaunchKernelGGL(fn[i], grid, dim3(threads), 0, st, a...);
  }
};

template <int NF, class... A>
inline PwKernelTable<NF, A...> pw_table(PwKernelTable<NF, A...> t) {
  const void* fs[NF];
  int n = 0;
  for (int i = 0; i < NF; ++i)
    if (t.counted >> i & 1) fs[n++] = reinterpret_cast<const void*>(t.fn[i]);
  t.occ = min_occupancy(fs, n, t.threads);
  return t;
}

// The path an exported pointwise operation takes, with that path's plan: the deep kernels before the
// streaming ones before the tiled engine (whose rows are stats_rows' / pwf_blocks': no plan).  Each
// row query and its entry read one function that returns this (gemm_pw.hip, pw_bwd_fused.hip,
// gemm_bf16.hip).
enum PwPath : int { kPwTiled = 0, kPwStream = 1, kPwDeep = 2 };
struct PwChoice {
  PwPath path;
  PwPlan plan;
};
static inline PwChoice pw_choice(PwPlan deep, PwPlan stream) {
  return deep.rows ? PwChoice{kPwDeep, deep} : stream.rows ? PwChoice{kPwStream, stream} : PwChoice{kPwTiled, {0, 0}};
}

// &k<leading..., flags...> for every value of n trailing bool flags, in index order
#define DK_PW_F1(k, ...) &k<__VA_ARGS__, false>, &k<__VA_ARGS__, true>
#define DK_PW_F2(k, ...) DK_PW_F1(k, __VA_ARGS__, false), DK_PW_F1(k, __VA_ARGS__, true)
#define DK_PW_F3(k, ...) DK_PW_F2(k, __VA_ARGS__, false), DK_PW_F2(k, __VA_ARGS__, true)
#define DK_PW_F4(k, ...) DK_PW_F3(k, __VA_ARGS__, false), DK_PW_F3(k, __VA_ARGS__, true)

}  // namespace dk
