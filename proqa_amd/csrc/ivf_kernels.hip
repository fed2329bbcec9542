// Inverted-file (IVF-Flat) search over fp16 [N,128] rows kept list-major in HBM.
//
// Replaces faiss.IndexIVFFlat(IndexFlatIP quantizer, 128, nlist) with the L2 metric, as the reference's
// qa/online_sampler.py:75-79 builds it and :274 searches it.  See DESIGN.md section 2.8.
//
//   ivf_coarse   one workgroup per query: the inner product with every float32 centroid (double accumulation,
//                rounded once), one LDS bitonic sort of (score, list) keys, the top nprobe lists; every (query, probe)
//                pair takes a rank in its list's bucket with one atomic (the per-list query counts the host reads back)
//   ivf_bucket   bucket[qoff[l] + rank] = q: the probes inverted into per-list query sets
//   ivf_scan     one workgroup per (list, 32 queries of its bucket, chunk of its rows).  The queries sit in registers as
//                MFMA B fragments; the rows stream through v_mfma_f32_32x32x16_f16 with the operand roles and k-step
//                order of mips_filter_f16 / bootstrap_scores (rows = A, queries = B, piece 2j+half at step j), so q.x
//                has the flat index's bits.  Rows rank by s = q.x - |x|^2/2 (argmin |q-x|^2 = argmax s: |q|^2 is
//                constant per query).  Each query keeps a running list of 2 k keys in LDS; a key enters when it beats
//                the k-th best key so far; a full list is sorted in place (bitonic) and cut to k.  The item writes
//                k sorted keys per query.
//   ivf_merge    one workgroup per query: its partial lists (one per probed list and chunk) in batches through an LDS
//                sort, the winners re-scored for q.x on the same MFMA sequence, D = max(|q|^2 - 2 s, 0), I = original id.
// Keys are (ord(score) << 32) | (0xFFFFFFFF - id): descending key order = score descending, id ascending.  Every key is a
// distinct row, so the result is the exact top k of the keys whatever the order in which workgroups ran.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "common.h"
#include "ivf_kernels.h"

namespace proqa {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRowBytes = 128 * 2;
constexpr int kScanWaves = 4;
constexpr int kRunKeys = 2 * kIvfMaxK;       // running list of one query in the scan
constexpr int kMergeKeys = 4096;             // keys one merge sorts at a time
constexpr int kMergeThreads = 256;

__device__ __forceinline__ unsigned ord_from_float(float f) {
  unsigned u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;  // -0.0 ties with +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_from_ord(unsigned o) {
  unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}
__device__ __forceinline__ unsigned long long pack_key(float score, unsigned id) {
  return ((unsigned long long)ord_from_float(score) << 32) | (unsigned long long)(0xFFFFFFFFu - id);
}

// Sorts keys[0, n) descending in segments of `seg` keys (n, seg powers of two, seg <= n); all T threads of the
// workgroup take part, and it ends with a barrier.
template <int T>
__device__ void bitonic_desc(unsigned long long* keys, int n, int seg, int tid) {
  for (int size = 2; size <= seg; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int p = tid; p < n / 2; p += T) {
        const int lo = 2 * p - (p & (stride - 1));
        const int hi = lo + stride;
        const bool desc = ((lo & (seg - 1)) & size) == 0;
        const unsigned long long a = keys[lo], b = keys[hi];
        if (desc ? a < b : a > b) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------
// add: list-major layout
// ---------------------------------------------------------------------------------------
// 16 threads per row (one 16-byte piece each); |x|^2 summed in double over the pieces in a fixed butterfly order
__global__ __launch_bounds__(256) void ivf_place_rows(const uint4* __restrict__ xb, const unsigned* __restrict__ sorted_list,
                                                      const unsigned* __restrict__ sorted_row, long long n,
                                                      const long long* __restrict__ dst_base, long long id0,
                                                      uint4* __restrict__ xs, float* __restrict__ hn, long long* __restrict__ ids,
                                                      long long* __restrict__ pos) {
  const long long i = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int piece = threadIdx.x & 15;
  double ss = 0.0;
  long long dst = 0, r = 0;
  if (i < n) {
    r = sorted_row[i];
    dst = dst_base[sorted_list[i]] + i;
    const uint4 v = xb[r * 16 + piece];
    xs[dst * 16 + piece] = v;
    const _Float16* h = (const _Float16*)&v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double f = (double)(float)h[e];
      ss += f * f;
    }
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 16);
  if (i < n && piece == 0) {
    hn[dst] = (float)(0.5 * ss);
    ids[dst] = id0 + r;
    pos[id0 + r] = dst;
  }
}

__global__ __launch_bounds__(256) void ivf_move_rows(const uint4* __restrict__ xs_old, const float* __restrict__ hn_old,
                                                     const long long* __restrict__ ids_old, long long n_old,
                                                     const long long* __restrict__ old_off, const long long* __restrict__ new_off,
                                                     int nlist, uint4* __restrict__ xs, float* __restrict__ hn,
                                                     long long* __restrict__ ids, long long* __restrict__ pos) {
  const long long p = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int piece = threadIdx.x & 15;
  if (p >= n_old) return;
  int lo = 0, hi = nlist - 1;   // the largest list l with old_off[l] <= p (it holds p: old_off[l + 1] > p)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (old_off[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  const long long dst = p - old_off[lo] + new_off[lo];
  xs[dst * 16 + piece] = xs_old[p * 16 + piece];
  if (piece == 0) {
    const long long id = ids_old[p];
    hn[dst] = hn_old[p];
    ids[dst] = id;
    pos[id] = dst;
  }
}

__global__ void ivf_histogram(const int* __restrict__ assign, long long n, unsigned* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(counts + assign[i], 1u);
}

__global__ void ivf_iota_kernel(unsigned* v, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (unsigned)i;
}

// ---------------------------------------------------------------------------------------
// search
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ivf_coarse(const _Float16* __restrict__ xq, const float* __restrict__ cent, int nlist,
                                                  int n_pow2, int nprobe, int* __restrict__ probes, int* __restrict__ rank,
                                                  float* __restrict__ qn2, unsigned* __restrict__ counts) {
  __shared__ unsigned long long keys[kIvfMaxList];
  __shared__ float s_q[128];
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  if (tid < 128) s_q[tid] = (float)xq[q * 128 + tid];
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int d = 0; d < 128; ++d) s += (double)s_q[d] * (double)s_q[d];
    qn2[q] = (float)s;
  }
  for (int c = tid; c < n_pow2; c += 256) {
    unsigned long long key = 0ull;
    if (c < nlist) {
      const float4* cr = (const float4*)(cent + (size_t)c * 128);
      double acc = 0.0;
#pragma unroll 4
      for (int d4 = 0; d4 < 32; ++d4) {
        const float4 v = cr[d4];
        acc += (double)v.x * (double)s_q[4 * d4] + (double)v.y * (double)s_q[4 * d4 + 1];
        acc += (double)v.z * (double)s_q[4 * d4 + 2] + (double)v.w * (double)s_q[4 * d4 + 3];
      }
      key = pack_key((float)acc, (unsigned)c);
    }
    keys[c] = key;
  }
  __syncthreads();
  bitonic_desc<256>(keys, n_pow2, n_pow2, tid);
  for (int p = tid; p < nprobe; p += 256) {
    const int l = (int)(0xFFFFFFFFu - (unsigned)keys[p]);
    probes[q * nprobe + p] = l;
    rank[q * nprobe + p] = (int)atomicAdd(counts + l, 1u);
  }
}

__global__ void ivf_bucket(const int* __restrict__ probes, const int* __restrict__ rank, long long n_pairs,
                           const int* __restrict__ qoff, int nprobe, int* __restrict__ bucket) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_pairs) bucket[qoff[probes[i]] + rank[i]] = (int)(i / nprobe);
}

// LDS state of one scan workgroup
struct ScanLds {
  unsigned long long run[kIvfTileQ * kRunKeys];   // 64 KiB: the running lists, query-major
  unsigned long long kth[kIvfTileQ];              // k-th best key of the query so far (0 until it has k)
  float tau[kIvfTileQ];                           // its score: the float pre-test of the MFMA results
  unsigned cnt[kIvfTileQ];                        // keys appended to the query's list (may pass kRunKeys: lost keys)
  float hn[kScanWaves][32];                       // |x|^2 / 2 of the rows of each wave's tile
  // a list ran over in this step, by step parity: every wave reads step i's flag after the barrier that ends step i, and
  // the next write of that flag comes in step i + 2, behind the barrier that ends step i + 1 -- which no wave passes before
  // every wave has read it (one flag for all steps would let a fast wave set it for step i + 1 before a slow wave has
  // read it for step i: that wave alone would then enter the list cut and its barriers)
  int over[2];
};

// sort every running list, cut it to k, publish the k-th key, clear the overflow flag of step parity `par`; every thread
// of the workgroup calls it, and it ends with a barrier
__device__ void scan_compact(ScanLds& s, unsigned k, int tid, int par) {
  for (int i = tid; i < kIvfTileQ * kRunKeys; i += kScanWaves * 64) {
    const unsigned n = min(s.cnt[i / kRunKeys], (unsigned)kRunKeys);
    if ((unsigned)(i % kRunKeys) >= n) s.run[i] = 0ull;
  }
  __syncthreads();
  bitonic_desc<kScanWaves * 64>(s.run, kIvfTileQ * kRunKeys, kRunKeys, tid);
  if (tid < kIvfTileQ) {
    const unsigned n = min(s.cnt[tid], k);
    s.cnt[tid] = n;
    if (n == k) {
      const unsigned long long kth = s.run[tid * kRunKeys + k - 1];
      s.kth[tid] = kth;
      s.tau[tid] = float_from_ord((unsigned)(kth >> 32));
    }
  }
  if (tid == 0) s.over[par] = 0;   // (every thread read it before the barriers above)
  __syncthreads();
}

__global__ __launch_bounds__(kScanWaves * 64, 2) void ivf_scan(const char* __restrict__ xs, const float* __restrict__ hn,
                                                               const long long* __restrict__ ids, const char* __restrict__ xq16,
                                                               const int* __restrict__ bucket, IvfListTable lt,
                                                               const IvfWork* __restrict__ work, int k,
                                                               unsigned long long* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) ScanLds s;
  const IvfWork w = work[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qb = lt.qoff[w.list] + w.qt * kIvfTileQ;
  const int nqt = min(kIvfTileQ, lt.qoff[w.list + 1] - qb);
  if (tid < kIvfTileQ) {
    s.kth[tid] = 0ull;
    s.tau[tid] = -3.402823466e38f;   // not -inf: a row holding +-inf or NaN scores -inf or NaN and must never enter (faiss' heap
                                     // takes d < FLT_MAX only)
    s.cnt[tid] = 0u;
  }
  if (tid == 0) s.over[0] = s.over[1] = 0;
  f16x8 qf[8];
  if (li < nqt) {
    const char* qp = xq16 + (size_t)bucket[qb + li] * kRowBytes;
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] = *(const f16x8*)(qp + (2 * j + half) * 16);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  const long long row0 = w.row0;
  const int n_rows = (int)(w.row1 - w.row0);
  const int n_tiles = (n_rows + 31) >> 5;
  const unsigned uk = (unsigned)k;
  __syncthreads();

  f16x8 af[8];
  float h = 0.f;
  auto load_tile = [&](int t, f16x8(&a)[8], float& hv) {
    const int rows_here = min(32, n_rows - t * 32);
    const long long arow = row0 + (long long)t * 32 + (li < rows_here ? li : rows_here - 1);
    const char* ap = xs + (size_t)arow * kRowBytes;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = *(const f16x8*)(ap + (2 * j + half) * 16);
    hv = hn[arow];
  };
  if (wave < n_tiles) load_tile(wave, af, h);

  for (int t0 = 0; t0 < n_tiles; t0 += kScanWaves) {
    const int par = (t0 / kScanWaves) & 1;
    const int t = t0 + wave;
    const bool mine = t < n_tiles;   // wave-uniform
    const bool more = t + kScanWaves < n_tiles;
    f16x8 an[8];
    float hnext = 0.f;
    float sc[16];
    unsigned lost = 0u;   // scores of this lane that passed but found its query's list full
    if (mine) {
      if (more) load_tile(t + kScanWaves, an, hnext);
      f32x16 acc = {0};
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[j], qf[j], acc, 0, 0, 0);
      // lane (li, half) holds query li, rows (r&3) + 8*(r>>2) + 4*half of the tile; LDS operations of one wave execute in
      // program order, so the reads below see the other lanes' writes
      if (half == 0) s.hn[wave][li] = h;
      const int rows_here = min(32, n_rows - t * 32);
      float m = __builtin_nanf("");
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rel = (r & 3) + 8 * (r >> 2) + 4 * half;
        sc[r] = rel < rows_here ? acc[r] - s.hn[wave][rel] : __builtin_nanf("");
        m = fmaxf(m, sc[r]);
      }
      if (li < nqt && m >= s.tau[li]) {
        const float tq = s.tau[li];
        const unsigned long long kth = s.kth[li];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (sc[r] >= tq) {
            const int rel = (r & 3) + 8 * (r >> 2) + 4 * half;
            const unsigned long long key = pack_key(sc[r], (unsigned)ids[row0 + (long long)t * 32 + rel]);
            if (key > kth) {
              const unsigned p = atomicAdd(&s.cnt[li], 1u);
              if (p < (unsigned)kRunKeys) {
                s.run[li * kRunKeys + p] = key;
              } else {
                lost |= 1u << r;
                s.over[par] = 1;
              }
            }
          }
        }
      }
    }
    __syncthreads();
    if (s.over[par]) {
      // a list overflowed: cut every list to its best k (the keys it holds), then append the keys that did not fit and
      // still beat the new k-th key; a list holds at most k keys after the cut and gains at most 128 -- it cannot overflow
      // again in this step
      scan_compact(s, uk, tid, par);
      if (lost) {
        const float tq = s.tau[li];
        const unsigned long long kth = s.kth[li];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (((lost >> r) & 1u) && sc[r] >= tq) {
            const int rel = (r & 3) + 8 * (r >> 2) + 4 * half;
            const unsigned long long key = pack_key(sc[r], (unsigned)ids[row0 + (long long)t * 32 + rel]);
            if (key > kth) s.run[li * kRunKeys + atomicAdd(&s.cnt[li], 1u)] = key;
          }
        }
      }
      __syncthreads();
    }
    if (mine && more) {
#pragma unroll
      for (int j = 0; j < 8; ++j) af[j] = an[j];
      h = hnext;
    }
  }
  scan_compact(s, uk, tid, 0);
  const long long nch = lt.nch[w.list];
  const long long slot0 = lt.slot0[w.list];
  for (int e = tid; e < nqt * k; e += kScanWaves * 64) {
    const int qi = e / k, j = e - qi * k;
    const long long slot = slot0 + (long long)(w.qt * kIvfTileQ + qi) * nch + w.chunk;
    partial[slot * k + j] = (unsigned)j < s.cnt[qi] ? s.run[qi * kRunKeys + j] : 0ull;
  }
}

__global__ __launch_bounds__(kMergeThreads) void ivf_merge(const unsigned long long* __restrict__ partial,
                                                           const int* __restrict__ probes, const int* __restrict__ rank,
                                                           int nprobe, IvfListTable lt, int k, const char* __restrict__ xs,
                                                           const long long* __restrict__ pos, const char* __restrict__ xq16,
                                                           const float* __restrict__ qn2, float* __restrict__ D,
                                                           long long* __restrict__ I, float* __restrict__ ip) {
  __shared__ __attribute__((aligned(16))) unsigned long long keys[kMergeKeys];
  __shared__ int s_pref[kIvfMaxProbe + 1];      // first partial list of probe p in this query's enumeration
  __shared__ long long s_base[kIvfMaxProbe];    // its slot
  __shared__ __attribute__((aligned(16))) char s_qrow[kRowBytes];
  __shared__ float s_sc[kMergeThreads / 64][32];
  __shared__ unsigned s_n;
  __shared__ unsigned long long s_kth;
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  if (tid == 0) {
    int acc = 0;
    for (int p = 0; p < nprobe; ++p) {
      const int l = probes[q * nprobe + p];
      s_pref[p] = acc;
      s_base[p] = lt.slot0[l] + (long long)rank[q * nprobe + p] * lt.nch[l];
      acc += lt.nch[l];
    }
    s_pref[nprobe] = acc;
    s_n = 0;
    s_kth = 0ull;
  }
  if (tid < kRowBytes / 16) ((uint4*)s_qrow)[tid] = ((const uint4*)(xq16 + q * kRowBytes))[tid];
  __syncthreads();
  const int n_lists = s_pref[nprobe];
  const int per_batch = (kMergeKeys - k) / k;
  unsigned run = 0;   // keys[0, run): the best keys so far, sorted
  for (int f0 = 0; f0 < n_lists; f0 += per_batch) {
    const int nl = min(per_batch, n_lists - f0);
    const unsigned long long kth = s_kth;
    for (int e = tid; e < nl * k; e += kMergeThreads) {
      const int f = f0 + e / k, j = e % k;
      int lo = 0, hi = nprobe - 1;   // the probe whose lists hold f: the largest p with s_pref[p] <= f
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_pref[mid] <= f) lo = mid;
        else hi = mid - 1;
      }
      const unsigned long long key = partial[(size_t)(s_base[lo] + (f - s_pref[lo])) * k + j];
      if (key > kth) keys[atomicAdd(&s_n, 1u)] = key;   // at most run + nl k <= kMergeKeys keys
    }
    __syncthreads();
    const unsigned n = s_n;
    // every thread holds n before any thread can start the next batch's appends to s_n (a batch that adds no key skips
    // the barriers below)
    __syncthreads();
    if (n > run) {
      int p2 = 2;
      while (p2 < (int)n) p2 <<= 1;
      for (int i = (int)n + tid; i < p2; i += kMergeThreads) keys[i] = 0ull;
      __syncthreads();
      bitonic_desc<kMergeThreads>(keys, p2, p2, tid);
      run = min(n, (unsigned)k);
      if (tid == 0) {
        s_n = run;
        if (run == (unsigned)k) s_kth = keys[k - 1];
      }
      __syncthreads();
    }
  }
  // re-score the winners: 32 per wave, the query in every B column (rescore_nominated_lists' layout), column 0 read back
  const int lane = tid & 63, wv = tid >> 6, li = lane & 31, half = lane >> 5;
  const int j0 = wv * 32;
  float ipv = -3.402823466e38f;
  if (j0 < (int)run) {   // wave-uniform
    const int j = j0 + li < (int)run ? j0 + li : j0;
    const unsigned id = 0xFFFFFFFFu - (unsigned)keys[j];
    const char* ap = xs + (size_t)pos[id] * kRowBytes;
    f16x8 af[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) af[jj] = *(const f16x8*)(ap + (2 * jj + half) * 16);
    f32x16 acc = {0};
    unsigned qoff = (unsigned)half * 16u;
    asm volatile("" : "+v"(qoff));
#pragma unroll
    for (int jj = 0; jj < 8; ++jj)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[jj], *(const f16x8*)(s_qrow + qoff + 32 * jj), acc, 0, 0, 0);
    if (li == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s_sc[wv][(r & 3) + 8 * (r >> 2) + 4 * half] = acc[r];
    }
    ipv = s_sc[wv][li];
  }
  const int j = j0 + li;
  if (half == 0 && j < k) {
    const size_t o = (size_t)q * k + j;
    if (j < (int)run) {
      const unsigned long long key = keys[j];
      const float sv = float_from_ord((unsigned)(key >> 32));
      // clamped at 0: |q|^2, q.x and |x|^2 / 2 are rounded separately, so a row (nearly) equal to the query can come out a few
      // ulps of |q|^2 below 0, which a squared distance never is; the ranking is by s, and the clamp keeps D monotone
      D[o] = fmaxf((float)((double)qn2[q] - 2.0 * (double)sv), 0.f);
      I[o] = (long long)(0xFFFFFFFFu - (unsigned)key);
      if (ip) ip[o] = ipv;
    } else {
      D[o] = 3.402823466e38f;
      I[o] = -1;
      if (ip) ip[o] = -3.402823466e38f;
    }
  }
}

__global__ __launch_bounds__(256) void ivf_gather(const uint4* __restrict__ xs, const long long* __restrict__ pos, long long n,
                                                  const long long* __restrict__ ids, long long n_ids, void* __restrict__ out,
                                                  int out_f32) {
  const long long i = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int piece = threadIdx.x & 15;
  if (i >= n_ids) return;
  const long long id = ids[i];
  uint4 v = {0u, 0u, 0u, 0u};
  if (id >= 0 && id < n) v = xs[pos[id] * 16 + piece];
  if (!out_f32) {
    ((uint4*)out)[i * 16 + piece] = v;
  } else {
    const _Float16* h = (const _Float16*)&v;
    float4* o = (float4*)out + i * 32 + piece * 2;
    o[0] = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
    o[1] = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
  }
}

}  // namespace

hipError_t launch_ivf_place_rows(const void* xb16, const unsigned* sorted_list, const unsigned* sorted_row, long long n,
                                 const long long* dst_base, long long id0, void* xs, float* hn, long long* ids, long long* pos,
                                 hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_place_rows, dim3((unsigned)ceil_div<long long>(n, 16)), dim3(256), 0, st, (const uint4*)xb16,
                     sorted_list, sorted_row, n, dst_base, id0, (uint4*)xs, hn, ids, pos);
  return hipGetLastError();
}

hipError_t launch_ivf_move_rows(const void* xs_old, const float* hn_old, const long long* ids_old, long long n_old,
                                const long long* old_off, const long long* new_off, int nlist, void* xs, float* hn,
                                long long* ids, long long* pos, hipStream_t st) {
  if (n_old <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_move_rows, dim3((unsigned)ceil_div<long long>(n_old, 16)), dim3(256), 0, st, (const uint4*)xs_old,
                     hn_old, ids_old, n_old, old_off, new_off, nlist, (uint4*)xs, hn, ids, pos);
  return hipGetLastError();
}

hipError_t launch_ivf_histogram(const int* assign, long long n, unsigned* counts, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_histogram, dim3((unsigned)ceil_div<long long>(n, 256)), dim3(256), 0, st, assign, n, counts);
  return hipGetLastError();
}

void ivf_iota(unsigned* v, long long n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(ivf_iota_kernel, dim3((unsigned)ceil_div<long long>(n, 256)), dim3(256), 0, st, v, n);
}

hipError_t ivf_sort_pairs(void* tmp, size_t* tmp_bytes, const unsigned* keys_in, unsigned* keys_out, const unsigned* vals_in,
                          unsigned* vals_out, int n, int bits, hipStream_t st) {
  return hipcub::DeviceRadixSort::SortPairs(tmp, *tmp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, bits, st);
}

hipError_t launch_ivf_coarse(const void* xq16, long long nq, const float* centroids, int nlist, int nprobe, int* probes,
                             int* rank, float* qn2, unsigned* counts, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  int n_pow2 = 2;
  while (n_pow2 < nlist) n_pow2 <<= 1;
  hipLaunchKernelGGL(ivf_coarse, dim3((unsigned)nq), dim3(256), 0, st, (const _Float16*)xq16, centroids, nlist, n_pow2, nprobe,
                     probes, rank, qn2, counts);
  return hipGetLastError();
}

hipError_t launch_ivf_bucket(const int* probes, const int* rank, long long nq, int nprobe, const int* qoff, int* bucket,
                             hipStream_t st) {
  const long long n_pairs = nq * nprobe;
  if (n_pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_bucket, dim3((unsigned)ceil_div<long long>(n_pairs, 256)), dim3(256), 0, st, probes, rank, n_pairs,
                     qoff, nprobe, bucket);
  return hipGetLastError();
}

hipError_t launch_ivf_scan(const void* xs, const float* hn, const long long* ids, const void* xq16, const int* bucket,
                           IvfListTable lt, const IvfWork* work, int n_work, int k, unsigned long long* partial,
                           hipStream_t st) {
  if (n_work <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_scan, dim3((unsigned)n_work), dim3(kScanWaves * 64), 0, st, (const char*)xs, hn, ids,
                     (const char*)xq16, bucket, lt, work, k, partial);
  return hipGetLastError();
}

hipError_t launch_ivf_merge(const unsigned long long* partial, const int* probes, const int* rank, long long nq, int nprobe,
                            IvfListTable lt, int k, const void* xs, const long long* pos, const void* xq16,
                            const float* qn2, float* D, long long* I, float* ip, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_merge, dim3((unsigned)nq), dim3(kMergeThreads), 0, st, partial, probes, rank, nprobe, lt, k,
                     (const char*)xs, pos, (const char*)xq16, qn2, D, I, ip);
  return hipGetLastError();
}

hipError_t launch_ivf_gather(const void* xs, const long long* pos, long long n, const long long* ids, long long n_ids,
                             void* out, bool out_f32, hipStream_t st) {
  if (n_ids <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_gather, dim3((unsigned)ceil_div<long long>(n_ids, 16)), dim3(256), 0, st, (const uint4*)xs, pos, n,
                     ids, n_ids, out, out_f32 ? 1 : 0);
  return hipGetLastError();
}

}  // namespace proqa
