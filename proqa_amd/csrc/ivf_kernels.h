// Launch interface between ivf_index.cpp (host orchestration) and ivf_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/proqa_hip.h"

namespace proqa {

constexpr int kIvfMaxK = 128;          // k of one search (the running lists of the scan hold 2 k keys per query)
constexpr int kIvfMaxList = 4096;      // nlist: the coarse step sorts one key per centroid in LDS
constexpr int kIvfMaxProbe = 1024;     // probes of one query that reach the scan (min(nprobe, nlist))
constexpr int kIvfTileQ = 32;          // queries of one scan work item (one MFMA B tile)

// One workgroup of ivf_scan: rows [row0, row1) of `list` (list-major positions) against the queries
// [qt * 32, qt * 32 + 32) of that list's bucket.  `chunk` is the index of the row range within the list.
struct IvfWork {
  int list;
  int chunk;
  int qt;
  int pad;
  long long row0;
  long long row1;
};
static_assert(sizeof(IvfWork) == 32, "work item layout");

// Per-list table of one search, uploaded once per search: bucket offsets (qoff, nlist + 1 entries), chunks of the list's
// rows (nch) and the first partial list of the list (slot0: the partial list of (query rank r, chunk c) is slot0 + r nch + c).
struct IvfListTable {
  const int* qoff;
  const int* nch;
  const long long* slot0;
};

// add: rows of one call, sorted stably by list (keys = list, vals = input row), placed behind the list's existing rows.
// dst_base[l] + i is the list-major position of the i-th sorted row of list l; id0 = ntotal before the call.
// Also writes hn = |x|^2 / 2 (double accumulation, rounded once), ids and the id -> position map.
hipError_t launch_ivf_place_rows(const void* xb16, const unsigned* sorted_list, const unsigned* sorted_row, long long n,
                                 const long long* dst_base, long long id0, void* xs, float* hn, long long* ids, long long* pos,
                                 hipStream_t st);
// moves the rows of the previous layout (old_off [nlist + 1]) to their place in the new one (new_off [nlist])
hipError_t launch_ivf_move_rows(const void* xs_old, const float* hn_old, const long long* ids_old, long long n_old,
                                const long long* old_off, const long long* new_off, int nlist, void* xs, float* hn,
                                long long* ids, long long* pos, hipStream_t st);
// counts[l] += rows of `assign` in list l
hipError_t launch_ivf_histogram(const int* assign, long long n, unsigned* counts, hipStream_t st);
void ivf_iota(unsigned* v, long long n, hipStream_t st);
// stable sort of (keys, vals) pairs by the low `bits` bits of the keys (hipcub radix sort); tmp == NULL: *tmp_bytes is set
hipError_t ivf_sort_pairs(void* tmp, size_t* tmp_bytes, const unsigned* keys_in, unsigned* keys_out, const unsigned* vals_in,
                          unsigned* vals_out, int n, int bits, hipStream_t st);

// coarse step: for every query the nprobe best lists by inner product with the float32 centroids (double accumulation,
// rounded once; ties to the lowest list), its rank in each probed list's bucket (counts[l] counts the queries of list l)
// and |q|^2 (same rounding).
hipError_t launch_ivf_coarse(const void* xq16, long long nq, const float* centroids, int nlist, int nprobe, int* probes,
                             int* rank, float* qn2, unsigned* counts, hipStream_t st);
// bucket[qoff[l] + rank] = q for every (q, probe)
hipError_t launch_ivf_bucket(const int* probes, const int* rank, long long nq, int nprobe, const int* qoff, int* bucket,
                             hipStream_t st);
// one workgroup per work item: the top-k keys (score s = q.x - |x|^2/2 descending, original id ascending) of the rows of the
// item for each of its queries, k keys per (query, chunk), 0 = no row
hipError_t launch_ivf_scan(const void* xs, const float* hn, const long long* ids, const void* xq16, const int* bucket,
                           IvfListTable lt, const IvfWork* work, int n_work, int k, unsigned long long* partial,
                           hipStream_t st);
// one workgroup per query: merges its partial lists, re-scores the winners (q.x, the flat index's MFMA sequence) and writes
// D = |q|^2 - 2 s, I = id and, when ip != NULL, the inner products
hipError_t launch_ivf_merge(const unsigned long long* partial, const int* probes, const int* rank, long long nq, int nprobe,
                            IvfListTable lt, int k, const void* xs, const long long* pos, const void* xq16,
                            const float* qn2, float* D, long long* I, float* ip, hipStream_t st);
// out[i] = row ids[i] (zero row for ids outside [0, n)), fp16 or float32
hipError_t launch_ivf_gather(const void* xs, const long long* pos, long long n, const long long* ids, long long n_ids,
                             void* out, bool out_f32, hipStream_t st);

}  // namespace proqa
