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
// inbatch_eval_blocks (the block-diagonal training objective, proqa_inbatch_loss_blocks_f16): the same body -- one text,
// inbatch_eval_body.h, included by both kernels -- on the square rectangle of each row block, the block on blockIdx.z and
// never split; inbatch_block_loss folds a block's lse - gold into its mean in a fixed order.
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
#include "inbatch_eval_body.h"
}

// ---- the block-diagonal objective --------------------------------------------------------------------------------------------
// Block m owns the rows [o[m], o[m + 1]) of q AND of c (BlockOffsets, common.h): its own square rectangle with the gold on
// the diagonal.
// grid (query tiles of the largest block, 1, blocks): workgroup (x, ., m) runs inbatch_eval_body on block m's slices as the
// single launch without a column split does (tiles_per_split = every column tile), so a workgroup never holds rows of two
// blocks and every lse / gold has the bits of that launch.  Workgroups past a smaller block's last query tile leave at once.
__global__ __launch_bounds__(kWaves * 64) void inbatch_eval_blocks(const char* __restrict__ q_all, const char* __restrict__ c_all,
                                                                   BlockOffsets offs, float* __restrict__ gold_all,
                                                                   float* __restrict__ lse_all) {
  const int block = blockIdx.z;
  const int o = offs.o[block], n = offs.o[block + 1] - o;
  if ((int)blockIdx.x * kTile >= n) return;           // the whole workgroup, before any barrier
  // what the single launch is handed for this rectangle
  const char* __restrict__ q = q_all + (size_t)o * kRowBytes;
  const char* __restrict__ c = c_all + (size_t)o * kRowBytes;
  const int* __restrict__ target = nullptr;
  const int nq = n, nc = n, tiles_per_split = (n + kTile - 1) / kTile;
  int* __restrict__ argmax_out = nullptr;
  int* __restrict__ rank_out = nullptr;
  float* __restrict__ max_out = nullptr;
  float* __restrict__ gold_out = gold_all + o;
  float* __restrict__ lse_out = lse_all + o;
  Partial* __restrict__ partial = nullptr;
#include "inbatch_eval_body.h"
}

// loss_out[m] = mean over block m's rows of lse - gold: one wave per block, lane l sums the rows l, l + 64, ... in order,
// then the lanes fold as a fixed tree.  No atomics: the same bits every run.
__global__ __launch_bounds__(64) void inbatch_block_loss(const float* __restrict__ lse, const float* __restrict__ gold,
                                                         BlockOffsets offs, float* __restrict__ loss_out) {
  const int m = blockIdx.x;
  const int o = offs.o[m], n = offs.o[m + 1] - o;
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) s += lse[o + i] - gold[o + i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (threadIdx.x == 0) loss_out[m] = s / (float)n;
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

int proqa_inbatch_loss_blocks_f16(const void* q, const void* c, const int32_t* block_offsets, int n_blocks, int n, int dim,
                                  float* lse_out, float* gold_out, float* loss_out, void* stream) {
  BlockOffsets offs;
  int widest = 0;
  const int rc = check_inbatch_blocks("inbatch_loss_blocks", block_offsets, n_blocks, n, dim, &offs, &widest);
  if (rc != PROQA_OK) return rc;
  if (!q || !c || !lse_out || !gold_out || !loss_out) return fail(PROQA_EINVAL, "inbatch_loss_blocks: NULL argument");
  if (!aligned16(q) || !aligned16(c)) return fail(PROQA_EINVAL, "inbatch_loss_blocks: q / c must be 16-byte aligned");
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(inbatch_eval_blocks, dim3((unsigned)ceil_div(widest, kTile), 1u, (unsigned)n_blocks), dim3(kWaves * 64), 0,
                     st, (const char*)q, (const char*)c, offs, gold_out, lse_out);
  PROQA_LAUNCH_CHECK();
  hipLaunchKernelGGL(inbatch_block_loss, dim3((unsigned)n_blocks), dim3(64), 0, st, (const float*)lse_out,
                     (const float*)gold_out, offs, loss_out);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

}  // extern "C"
