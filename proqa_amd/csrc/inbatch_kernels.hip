// In-batch scoring of the retriever's dev evaluation and training objective: product = q @ c.T over one collated batch,
// product.argmax(-1) against the gold column and CrossEntropyLoss(product, target) (retrieval/train_retriever.py:203-205,
// 318-323).  The reference forms the [nq, nc] product; here it never exists in memory.
//
// inbatch_eval: a workgroup of four waves owns 32 query rows.  Every wave keeps the rows' 8 MFMA B fragments in registers
// for its lifetime and walks its share of the 32-passage column tiles (tile w, w + 4, ... of the workgroup's column range)
// on v_mfma_f32_32x32x16_f16 -- the shape, operand roles and k-step order of mips_filter_f16 (passages = A, queries = B,
// piece 2j + half at step j), so a (query, passage) score has the bits the exact search reports for that pair.  The
// accumulator puts a query on the lane and 16 of the tile's 32 passages in the lane's registers, so the per-row state
//     (max, argmax, columns that beat the gold, running sum of exp(s - max), first NaN column)
// is per lane and the inner loop moves nothing between lanes.  The gold score s[i, target[i]] is needed before the count:
// every wave starts with one more 32 x 32 tile whose A rows are gathered through target[] and keeps its diagonal (the same
// instruction sequence on the same two rows: the same bits as the sweep gives that column).  The two lane halves, then the
// four waves (through LDS) are merged at the end.  When nq is small the column tiles are split over blockIdx.y; each split
// leaves its merged state in a workspace and inbatch_combine, one thread per row, folds the splits in order.
//
// Order of the scores (torch's, pinned by tests/inbatch_oracle.py): a NaN is greater than every number and NaNs are equal
// to each other; among equal scores the lowest column wins the argmax, and a column equal to the gold beats it only from
// the left.  A row with a NaN reports max = lse = NaN and the first NaN as its argmax.  lse follows torch.logsumexp: the
// maximum is subtracted unless it is infinite (a row holding +inf gives +inf, a row of -inf gives -inf).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>
#include <cmath>
#include <mutex>

#include "common.h"

namespace proqa {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRowBytes = PROQA_EMBED_DIM * 2;
constexpr int kWaves = 4;            // waves of a workgroup; they share the query tile and split its column tiles
constexpr int kTile = 32;            // query rows of a workgroup = passages of a column tile (the MFMA's M = N)
constexpr int kTargetGrid = 512;     // workgroups the column split aims for (two per CU)
constexpr int kMinTilesPerWave = 4;  // a split is not made finer than this many column tiles per wave
constexpr int kMaxSplitTiles = 1024; // (query tiles) x (splits) of a split launch: bounds the workspace
constexpr int kMaxRows = 1 << 24;    // of q and of c: column and tile arithmetic stays far inside int

struct RowState {
  float m;     // greatest non-NaN score so far (-inf: none)
  int arg;     // its lowest column (INT_MAX: none)
  int cnt;     // columns that beat the gold
  float sum;   // sum of exp(s - shift(m)) over the non-NaN scores
  int nan;     // lowest column with a NaN score (INT_MAX: none)
};

// torch.logsumexp's shift: the maximum, or 0 where that is infinite
__device__ __forceinline__ float shift_of(float m) { return fabsf(m) == INFINITY ? 0.f : m; }

// `sum`, accumulated against the maximum `from`, restated against the maximum `to` >= from.  sum == 0 exactly when
// from == -inf (nothing but -inf seen): left alone, 0 * exp(+large) would be NaN.
__device__ __forceinline__ float rescale(float sum, float from, float to) {
  return (from == to || sum == 0.f) ? sum : sum * expf(shift_of(from) - shift_of(to));
}

__device__ __forceinline__ void merge(RowState& a, const RowState& b) {
  const float mn = fmaxf(a.m, b.m);   // neither is NaN
  a.sum = rescale(a.sum, a.m, mn) + rescale(b.sum, b.m, mn);
  if (b.m > a.m || (b.m == a.m && b.arg < a.arg)) a.arg = b.arg;
  a.m = mn;
  a.cnt += b.cnt;
  a.nan = min(a.nan, b.nan);
}

__device__ __forceinline__ void finalize(const RowState& s, float gold, int target_ok, int row, int* __restrict__ argmax_out,
                                         int* __restrict__ rank_out, float* __restrict__ max_out, float* __restrict__ gold_out,
                                         float* __restrict__ lse_out) {
  const bool has_nan = s.nan != INT_MAX;
  if (argmax_out) argmax_out[row] = has_nan ? s.nan : s.arg;
  if (rank_out) rank_out[row] = target_ok ? s.cnt : -1;
  if (max_out) max_out[row] = has_nan ? NAN : s.m;
  if (gold_out) gold_out[row] = gold;
  if (lse_out) lse_out[row] = has_nan ? NAN : logf(s.sum) + shift_of(s.m);
}

// the 8 operand fragments of one row for lane half `half`: 16-byte piece 2j + half at k-step j
__device__ __forceinline__ void load_frags(f16x8 (&f)[8], const char* __restrict__ row, int half) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = *(const f16x8*)(row + (2 * j + half) * 16);
}

struct Partial {   // one split's merged state of one query row (workspace of the split launch)
  float m, sum;
  int arg, cnt, nan;
};

// grid (query tiles, splits).  Split y owns the column tiles [y * tiles_per_split, (y + 1) * tiles_per_split).
__global__ __launch_bounds__(kWaves * 64) void inbatch_eval(const char* __restrict__ q, const char* __restrict__ c,
                                                            const int* __restrict__ target, int nq, int nc, int tiles_per_split,
                                                            int* __restrict__ argmax_out, int* __restrict__ rank_out,
                                                            float* __restrict__ max_out, float* __restrict__ gold_out,
                                                            float* __restrict__ lse_out, Partial* __restrict__ partial) {
  __shared__ RowState red[kWaves][kTile];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, half = lane >> 5;
  const int row = blockIdx.x * kTile + li;            // this lane's query row; rows >= nq compute on row nq - 1, unwritten
  const int lrow = row < nq ? row : nq - 1;
  f16x8 qf[8];
  load_frags(qf, q + (size_t)lrow * kRowBytes, half);

  // gold: A row li = passage target[query li]; the diagonal element (li, li) sits in the lane half (li >> 2) & 1 at
  // register (li & 3) + 4 * (li >> 3)
  const int t = target ? target[lrow] : lrow;
  const int target_ok = t >= 0 && t < nc;
  float gold;
  {
    f16x8 af[8];
    load_frags(af, c + (size_t)(target_ok ? t : 0) * kRowBytes, half);
    f32x16 acc = {0};
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[j], qf[j], acc, 0, 0, 0);
    const int dreg = (li & 3) + 4 * (li >> 3);
    float d = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) d = r == dreg ? acc[r] : d;
    const float other = __shfl_xor(d, 32, 64);
    gold = ((li >> 2) & 1) == half ? d : other;
    if (!target_ok) gold = NAN;   // a target outside [0, nc): gold NaN, rank -1
  }
  const bool gold_nan = gold != gold;

  RowState st = {-INFINITY, INT_MAX, 0, 0.f, INT_MAX};
  const int n_tiles = (nc + kTile - 1) / kTile;
  const int tile_lo = blockIdx.y * tiles_per_split;
  const int tile_hi = min(n_tiles, tile_lo + tiles_per_split);
  // the next tile's fragments are requested before the current tile's arithmetic
  f16x8 af[8], nf[8];
  int tile = tile_lo + wave;
  if (tile < tile_hi) load_frags(af, c + (size_t)min(tile * kTile + li, nc - 1) * kRowBytes, half);
  for (; tile < tile_hi; tile += kWaves) {
    const int next = tile + kWaves;
    if (next < tile_hi) load_frags(nf, c + (size_t)min(next * kTile + li, nc - 1) * kRowBytes, half);
    f32x16 acc = {0};
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[j], qf[j], acc, 0, 0, 0);
    // register r of lane (li, half): query li, passage (r & 3) + 8 (r >> 2) + 4 half of the tile -- increasing in r, and
    // a wave's tiles increase, so a strict > keeps the lowest column of equal scores
    const int col0 = tile * kTile + 4 * half;
    float tm = st.m;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int col = col0 + (r & 3) + 8 * (r >> 2);
      const float s = acc[r];
      if (col < nc) {
        const bool s_nan = s != s;
        if (s_nan) {
          st.nan = min(st.nan, col);
        } else if (s > tm || (s == tm && col < st.arg)) {   // (the second clause: the row's first -inf)
          tm = s;
          st.arg = col;
        }
        const bool gt = s_nan ? !gold_nan : s > gold;
        const bool eq = s_nan ? gold_nan : s == gold;
        st.cnt += (col != t && (gt || (eq && col < t))) ? 1 : 0;
      }
    }
    float sum = rescale(st.sum, st.m, tm);
    const float sh = shift_of(tm);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int col = col0 + (r & 3) + 8 * (r >> 2);
      const float s = acc[r];
      if (col < nc && s == s) sum += expf(s - sh);
    }
    st.sum = sum;
    st.m = tm;
    if (next < tile_hi) {
#pragma unroll
      for (int j = 0; j < 8; ++j) af[j] = nf[j];
    }
  }

  // the other lane half holds the other 16 passages of every tile
  {
    RowState o;
    o.m = __shfl_xor(st.m, 32, 64);
    o.arg = __shfl_xor(st.arg, 32, 64);
    o.cnt = __shfl_xor(st.cnt, 32, 64);
    o.sum = __shfl_xor(st.sum, 32, 64);
    o.nan = __shfl_xor(st.nan, 32, 64);
    merge(st, o);
  }
  if (half == 0) red[wave][li] = st;
  __syncthreads();
  if (threadIdx.x < kTile) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) merge(st, red[w][li]);
    if (row < nq) {
      if (partial) {
        Partial p = {st.m, st.sum, st.arg, st.cnt, st.nan};
        partial[(size_t)blockIdx.y * nq + row] = p;
        if (blockIdx.y == 0 && gold_out) gold_out[row] = gold;
      } else {
        finalize(st, gold, target_ok, row, argmax_out, rank_out, max_out, gold_out, lse_out);
      }
    }
  }
}

// one thread per query row folds the splits in column order; gold_out was written by split 0
__global__ __launch_bounds__(256) void inbatch_combine(const Partial* __restrict__ partial, const int* __restrict__ target,
                                                       int nq, int nc, int n_split, int* __restrict__ argmax_out,
                                                       int* __restrict__ rank_out, float* __restrict__ max_out,
                                                       float* __restrict__ lse_out) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nq) return;
  RowState st = {-INFINITY, INT_MAX, 0, 0.f, INT_MAX};
  for (int y = 0; y < n_split; ++y) {
    const Partial p = partial[(size_t)y * nq + row];
    const RowState o = {p.m, p.arg, p.cnt, p.sum, p.nan};
    merge(st, o);
  }
  const int t = target ? target[row] : row;
  finalize(st, 0.f, t >= 0 && t < nc, row, argmax_out, rank_out, max_out, nullptr, lse_out);
}

// Workspace of the split launch, one per device, allocated at the first split call on that device and kept: the split is
// only taken below kMaxSplitTiles (query tile, split) pairs, so its size is fixed.  Split calls of one device are ordered
// on the device: each records `done` behind its combine launch, and a call on another stream than the last one makes its
// stream wait for that event before it touches the partials.  The host side (look-up, wait, launches, record) runs under
// the mutex, so callers on several host threads are ordered too.
constexpr int kMaxDevices = 64;
struct SplitWorkspace {
  Partial* partial = nullptr;
  hipEvent_t done = nullptr;
  hipStream_t last = nullptr;
  bool used = false;
};
std::mutex g_ws_mutex;
SplitWorkspace g_ws[kMaxDevices];

// with g_ws_mutex held
int split_workspace(SplitWorkspace** out) {
  int dev = 0;
  PROQA_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices) return fail(PROQA_EINVAL, "inbatch_eval: device %d out of range", dev);
  SplitWorkspace& w = g_ws[dev];
  if (!w.partial) {
    void* p = nullptr;
    if (try_malloc(&p, (size_t)kMaxSplitTiles * kTile * sizeof(Partial)) != hipSuccess)
      return fail(PROQA_ENOMEM, "inbatch_eval: workspace allocation failed");
    const hipError_t e = hipEventCreateWithFlags(&w.done, hipEventDisableTiming);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return hip_fail(e, "hipEventCreateWithFlags", __FILE__, __LINE__);
    }
    w.partial = (Partial*)p;
  }
  *out = &w;
  return PROQA_OK;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace proqa

using namespace proqa;

extern "C" {

int proqa_inbatch_eval_f16(const void* q, const void* c, const int32_t* target, int nq, int nc, int dim, int32_t* argmax_out,
                           int32_t* rank_out, float* max_out, float* gold_out, float* lse_out, void* stream) {
  if (dim != PROQA_EMBED_DIM) return fail(PROQA_EINVAL, "inbatch_eval: dim=%d, only %d is supported", dim, PROQA_EMBED_DIM);
  if (nq < 0 || nc < 0 || nq > kMaxRows || nc > kMaxRows)
    return fail(PROQA_EINVAL, "inbatch_eval: bad sizes nq=%d nc=%d (at most %d each)", nq, nc, kMaxRows);
  if (nq == 0) return PROQA_OK;
  if (nc == 0) return fail(PROQA_EINVAL, "inbatch_eval: nq=%d rows against no column", nq);
  if (!target && nq > nc)
    return fail(PROQA_EINVAL, "inbatch_eval: target == NULL means target[i] = i and needs nq <= nc (nq=%d nc=%d)", nq, nc);
  if (!q || !c) return fail(PROQA_EINVAL, "inbatch_eval: NULL argument");
  if (!aligned16(q) || !aligned16(c)) return fail(PROQA_EINVAL, "inbatch_eval: q / c must be 16-byte aligned");
  if (!argmax_out && !rank_out && !max_out && !gold_out && !lse_out) return PROQA_OK;

  const int q_tiles = ceil_div(nq, kTile), c_tiles = ceil_div(nc, kTile);
  // splits: enough workgroups for the device, no finer than kMinTilesPerWave column tiles per wave
  int n_split = 1;
  if (q_tiles < kTargetGrid) {
    n_split = std::min(ceil_div(kTargetGrid, q_tiles), ceil_div(c_tiles, kWaves * kMinTilesPerWave));
    n_split = std::max(1, std::min(n_split, kMaxSplitTiles / q_tiles));
  }
  const int tiles_per_split = ceil_div(c_tiles, n_split);
  n_split = ceil_div(c_tiles, tiles_per_split);   // no empty split
  const hipStream_t st = as_stream(stream);
  if (n_split == 1) {
    hipLaunchKernelGGL(inbatch_eval, dim3((unsigned)q_tiles, 1u), dim3(kWaves * 64), 0, st, (const char*)q, (const char*)c,
                       (const int*)target, nq, nc, tiles_per_split, (int*)argmax_out, (int*)rank_out, max_out, gold_out,
                       lse_out, (Partial*)nullptr);
    PROQA_LAUNCH_CHECK();
    return PROQA_OK;
  }
  std::lock_guard<std::mutex> lock(g_ws_mutex);
  SplitWorkspace* ws = nullptr;
  const int rc = split_workspace(&ws);
  if (rc != PROQA_OK) return rc;
  if (ws->used && ws->last != st) PROQA_HIP(hipStreamWaitEvent(st, ws->done, 0));   // the partials are still another stream's
  hipLaunchKernelGGL(inbatch_eval, dim3((unsigned)q_tiles, (unsigned)n_split), dim3(kWaves * 64), 0, st, (const char*)q,
                     (const char*)c, (const int*)target, nq, nc, tiles_per_split, (int*)argmax_out, (int*)rank_out, max_out,
                     gold_out, lse_out, ws->partial);
  PROQA_LAUNCH_CHECK();
  hipLaunchKernelGGL(inbatch_combine, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, st, (const Partial*)ws->partial,
                     (const int*)target, nq, nc, n_split, (int*)argmax_out, (int*)rank_out, max_out, lse_out);
  PROQA_LAUNCH_CHECK();
  PROQA_HIP(hipEventRecord(ws->done, st));
  ws->last = st;
  ws->used = true;
  return PROQA_OK;
}

}  // extern "C"
