// proqa_ivf: the inverted-file index (faiss IndexIVFFlat, L2 lists behind an inner-product quantizer) -- host side.
//
// Layout (after every add): the rows of all lists in ONE list-major fp16 copy xs [ntotal, 128], list l at positions
// [off[l], off[l + 1]), each list in add order (= ascending original id); next to it hn = |x|^2 / 2 (float32), the
// original id of every position and the position of every id.  An add re-lays the whole index out (old rows first in
// every list, then the new ones in input order), so several adds give the layout of one add of their concatenation.
//
// A search: coarse kernel -> ONE device-to-host copy of the per-list query counts (the only host wait) -> work items built
// on the host and uploaded -> bucket, scan and merge kernels.  Nothing else crosses to the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "ivf_kernels.h"
#include "mips_kernels.h"

using namespace proqa;

struct proqa_ivf {
  int device = 0;
  int nlist = 0;
  int allow_rounding = 0;
  float* cent = nullptr;           // [nlist, 128] float32
  bool trained = false;
  long long ntotal = 0;
  std::vector<long long> off;      // [nlist + 1] list offsets (host copy)
  long long* off_dev = nullptr;    // [nlist + 1]
  void* xs = nullptr;              // fp16 [ntotal, 128] list-major
  float* hn = nullptr;             // [ntotal]
  long long* ids = nullptr;        // [ntotal] original id of each position
  long long* pos = nullptr;        // [ntotal] position of each original id
  // search workspace (grow-only; see proqa_hip.h for the bound)
  struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
  };
  Buf w_xq, w_probes, w_rank, w_qn2, w_counts, w_bucket, w_table, w_work, w_partial;
  unsigned* counts_host = nullptr;  // pinned [nlist + 2]: per-list query counts, the two conversion flags
  std::vector<IvfWork> work;
  std::vector<char> table;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  proqa_ivf_stats stats = {};
  bool stats_pending = false;
};

namespace {

int ensure(proqa_ivf::Buf& b, size_t bytes) {
  if (bytes <= b.bytes) return PROQA_OK;
  if (b.p) PROQA_HIP(hipFree(b.p));
  b.p = nullptr;
  b.bytes = 0;
  if (try_malloc(&b.p, bytes) != hipSuccess) return fail(PROQA_ENOMEM, "ivf: cannot allocate %zu bytes of workspace", bytes);
  b.bytes = bytes;
  return PROQA_OK;
}

void free_layout(proqa_ivf* h) {
  void* ptrs[] = {h->xs, h->hn, h->ids, h->pos};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  h->xs = nullptr;
  h->hn = nullptr;
  h->ids = nullptr;
  h->pos = nullptr;
}

constexpr long long kAddPiece = 1ll << 24;   // rows per k-means assign call of an add

}  // namespace

extern "C" {

int proqa_ivf_free(proqa_ivf* h) {
  if (!h) return PROQA_OK;
  free_layout(h);
  if (h->cent) (void)hipFree(h->cent);
  if (h->off_dev) (void)hipFree(h->off_dev);
  proqa_ivf::Buf* bufs[] = {&h->w_xq, &h->w_probes, &h->w_rank, &h->w_qn2, &h->w_counts, &h->w_bucket, &h->w_table, &h->w_work,
                            &h->w_partial};
  for (auto* b : bufs)
    if (b->p) (void)hipFree(b->p);
  if (h->counts_host) (void)hipHostFree(h->counts_host);
  for (auto& e : h->ev)
    if (e) (void)hipEventDestroy(e);
  delete h;
  return PROQA_OK;
}

int proqa_ivf_create(int d, int nlist, proqa_ivf** out) {
  if (!out) return fail(PROQA_EINVAL, "ivf_create: out is NULL");
  *out = nullptr;
  if (d != PROQA_EMBED_DIM) return fail(PROQA_EINVAL, "ivf_create: d=%d, only d=128 is supported", d);
  if (nlist < 1 || nlist > kIvfMaxList) return fail(PROQA_EINVAL, "ivf_create: nlist=%d outside [1, %d]", nlist, kIvfMaxList);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PROQA_ENOGPU, "ivf_create: no HIP device");
  proqa_ivf* h = new (std::nothrow) proqa_ivf();
  if (!h) return fail(PROQA_ENOMEM, "ivf_create: out of host memory");
  PROQA_HIP(hipGetDevice(&h->device));
  h->nlist = nlist;
  h->off.assign((size_t)nlist + 1, 0);
  hipError_t e = hipMalloc((void**)&h->cent, (size_t)nlist * PROQA_EMBED_DIM * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&h->off_dev, ((size_t)nlist + 1) * sizeof(long long));
  if (e == hipSuccess) e = hipMemset(h->off_dev, 0, ((size_t)nlist + 1) * sizeof(long long));
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->counts_host, ((size_t)nlist + 2) * sizeof(unsigned));
  for (auto& ev : h->ev)
    if (e == hipSuccess) e = hipEventCreate(&ev);
  if (e != hipSuccess) {
    proqa_ivf_free(h);
    return fail(PROQA_ENOMEM, "ivf_create: allocation failed: %s", hipGetErrorString(e));
  }
  *out = h;
  return PROQA_OK;
}

int proqa_ivf_set_centroids(proqa_ivf* h, const float* centroids_dev) {
  if (!h || !centroids_dev) return fail(PROQA_EINVAL, "ivf_set_centroids: NULL argument");
  if (h->ntotal) return fail(PROQA_EINVAL, "ivf_set_centroids: the index holds rows (reset it first)");
  PROQA_ON_DEVICE(h->device);
  PROQA_HIP(hipMemcpy(h->cent, centroids_dev, (size_t)h->nlist * PROQA_EMBED_DIM * sizeof(float), hipMemcpyDeviceToDevice));
  h->trained = true;
  return PROQA_OK;
}

int proqa_ivf_allow_rounding(proqa_ivf* h, int allow) {
  if (!h) return fail(PROQA_EINVAL, "ivf_allow_rounding: NULL handle");
  h->allow_rounding = allow ? 1 : 0;
  return PROQA_OK;
}

int proqa_ivf_reset(proqa_ivf* h) {
  if (!h) return fail(PROQA_EINVAL, "ivf_reset: NULL handle");
  PROQA_ON_DEVICE(h->device);
  PROQA_HIP(hipDeviceSynchronize());
  free_layout(h);
  h->ntotal = 0;
  std::fill(h->off.begin(), h->off.end(), 0ll);
  PROQA_HIP(hipMemset(h->off_dev, 0, ((size_t)h->nlist + 1) * sizeof(long long)));
  return PROQA_OK;
}

int proqa_ivf_ntotal(const proqa_ivf* h, int64_t* out) {
  if (!h || !out) return fail(PROQA_EINVAL, "ivf_ntotal: NULL argument");
  *out = h->ntotal;
  return PROQA_OK;
}

int proqa_ivf_list_sizes(const proqa_ivf* h, int64_t* sizes_out) {
  if (!h || !sizes_out) return fail(PROQA_EINVAL, "ivf_list_sizes: NULL argument");
  for (int l = 0; l < h->nlist; ++l) sizes_out[l] = h->off[l + 1] - h->off[l];
  return PROQA_OK;
}

int proqa_ivf_list_ids(const proqa_ivf* h, int64_t* ids_out) {
  if (!h || !ids_out) return fail(PROQA_EINVAL, "ivf_list_ids: NULL argument");
  if (!h->ntotal) return PROQA_OK;
  PROQA_ON_DEVICE(h->device);
  PROQA_HIP(hipDeviceSynchronize());
  PROQA_HIP(hipMemcpy(ids_out, h->ids, (size_t)h->ntotal * sizeof(long long), hipMemcpyDeviceToHost));
  return PROQA_OK;
}

int proqa_ivf_add_device(proqa_ivf* h, const void* xb_f16_dev, int64_t n, void* stream) {
  if (!h || (!xb_f16_dev && n > 0)) return fail(PROQA_EINVAL, "ivf_add: NULL argument");
  if (!h->trained) return fail(PROQA_EINVAL, "ivf_add: the index is not trained (set the centroids first)");
  if (n < 0 || n >= (1ll << 31)) return fail(PROQA_EINVAL, "ivf_add: n=%lld outside [0, 2^31)", (long long)n);
  if (h->ntotal + n >= 0xFFFFFFFFll) return fail(PROQA_EINVAL, "ivf_add: more than 2^32 - 2 rows in one index");
  if (n == 0) return PROQA_OK;
  PROQA_ON_DEVICE(h->device);
  hipStream_t st = as_stream(stream);
  const int nlist = h->nlist;
  const long long n_old = h->ntotal, n_new = n_old + n;
  // 1. list of every new row: nearest centroid by inner product, ties to the lowest list (the k-means assign)
  int* assign = nullptr;
  float* dist = nullptr;
  unsigned *keys_out = nullptr, *vals_in = nullptr, *vals_out = nullptr, *counts = nullptr;
  long long* base_dev = nullptr;
  void* sort_tmp = nullptr;
  void *xs = nullptr;
  float* hn = nullptr;
  long long *ids = nullptr, *pos = nullptr, *new_off_dev = nullptr;
  proqa_kmeans* km = nullptr;
  int rc = PROQA_OK;
  auto cleanup = [&]() {
    void* ptrs[] = {assign, dist, keys_out, vals_in, vals_out, counts, base_dev, sort_tmp, new_off_dev};
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
    if (km) proqa_kmeans_free(km);
  };
  auto bail = [&](int code) {
    cleanup();
    void* lay[] = {xs, hn, ids, pos};
    for (void* p : lay)
      if (p) (void)hipFree(p);
    return code;
  };
  hipError_t e = hipSuccess;
  auto alloc = [&](void** p, size_t bytes) {
    if (e == hipSuccess) e = try_malloc(p, bytes);
  };
  const long long piece = std::min<long long>(n, kAddPiece);
  alloc((void**)&assign, (size_t)n * sizeof(int));
  alloc((void**)&dist, (size_t)piece * sizeof(float));
  alloc((void**)&keys_out, (size_t)n * sizeof(unsigned));
  alloc((void**)&vals_in, (size_t)n * sizeof(unsigned));
  alloc((void**)&vals_out, (size_t)n * sizeof(unsigned));
  alloc((void**)&counts, (size_t)nlist * sizeof(unsigned));
  alloc((void**)&base_dev, (size_t)nlist * sizeof(long long));
  alloc((void**)&new_off_dev, ((size_t)nlist + 1) * sizeof(long long));
  alloc(&xs, (size_t)n_new * kDim * 2);
  alloc((void**)&hn, (size_t)n_new * sizeof(float));
  alloc((void**)&ids, (size_t)n_new * sizeof(long long));
  alloc((void**)&pos, (size_t)n_new * sizeof(long long));
  if (e != hipSuccess) return bail(fail(PROQA_ENOMEM, "ivf_add: device allocation failed: %s", hipGetErrorString(e)));
  if ((rc = proqa_kmeans_create(kDim, piece, nlist, &km)) != PROQA_OK) return bail(rc);
  for (long long r0 = 0; r0 < n; r0 += piece) {
    const long long m = std::min(piece, n - r0);
    if ((rc = proqa_kmeans_assign_device(km, (const char*)xb_f16_dev + (size_t)r0 * kDim * 2, m, h->cent, 0, assign + r0,
                                         dist, stream)) != PROQA_OK)
      return bail(rc);
  }
  // 2. stable sort of the new rows by list, list sizes
  int bits = 1;
  while ((1 << bits) < nlist) ++bits;
  size_t tmp_bytes = 0;
  if ((e = ivf_sort_pairs(nullptr, &tmp_bytes, (const unsigned*)assign, keys_out, vals_in, vals_out, (int)n, bits, st)) != hipSuccess ||
      (e = try_malloc(&sort_tmp, tmp_bytes)) != hipSuccess)
    return bail(fail(PROQA_ENOMEM, "ivf_add: sort workspace: %s", hipGetErrorString(e)));
  ivf_iota(vals_in, n, st);
  if ((e = ivf_sort_pairs(sort_tmp, &tmp_bytes, (const unsigned*)assign, keys_out, vals_in, vals_out, (int)n, bits, st)) != hipSuccess ||
      (e = hipMemsetAsync(counts, 0, (size_t)nlist * sizeof(unsigned), st)) != hipSuccess ||
      (e = launch_ivf_histogram(assign, n, counts, st)) != hipSuccess)
    return bail(hip_fail(e, "ivf_add: sort", __FILE__, __LINE__));
  std::vector<unsigned> cnt(nlist);
  if ((e = hipMemcpyAsync(cnt.data(), counts, (size_t)nlist * sizeof(unsigned), hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess)
    return bail(hip_fail(e, "ivf_add: list counts", __FILE__, __LINE__));
  // 3. new offsets; sorted row i of list l goes to new_off[l] + old size of l + (i - first sorted row of l)
  std::vector<long long> new_off((size_t)nlist + 1), base(nlist);
  long long acc = 0, first = 0;
  for (int l = 0; l < nlist; ++l) {
    new_off[l] = acc;
    const long long old_size = h->off[l + 1] - h->off[l];
    base[l] = acc + old_size - first;
    first += cnt[l];
    acc += old_size + cnt[l];
  }
  new_off[nlist] = acc;
  if ((e = hipMemcpyAsync(base_dev, base.data(), (size_t)nlist * sizeof(long long), hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(new_off_dev, new_off.data(), ((size_t)nlist + 1) * sizeof(long long), hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = launch_ivf_move_rows(h->xs, h->hn, h->ids, n_old, h->off_dev, new_off_dev, nlist, xs, hn, ids, pos, st)) != hipSuccess ||
      (e = launch_ivf_place_rows(xb_f16_dev, keys_out, vals_out, n, base_dev, n_old, xs, hn, ids, pos, st)) != hipSuccess ||
      (e = hipMemcpyAsync(h->off_dev, new_off_dev, ((size_t)nlist + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess)
    return bail(hip_fail(e, "ivf_add: layout", __FILE__, __LINE__));
  cleanup();
  free_layout(h);
  h->xs = xs;
  h->hn = hn;
  h->ids = ids;
  h->pos = pos;
  h->off = new_off;
  h->ntotal = n_new;
  return PROQA_OK;
}

int proqa_ivf_search_device(proqa_ivf* h, const void* xq_dev, int dtype, int64_t nq, int k, int nprobe, float* D_dev,
                            int64_t* I_dev, float* ip_dev, void* stream) {
  if (!h) return fail(PROQA_EINVAL, "ivf_search: NULL handle");
  // the statistics describe this call from here on: one that fails or is refused leaves them zero (never the events of two
  // different searches)
  h->stats = proqa_ivf_stats{};
  h->stats_pending = false;
  if (k < 1 || k > kIvfMaxK)
    return fail(PROQA_EINVAL, "ivf_search: k=%d outside [1, %d] (IndexFlatIP searches any k)", k, kIvfMaxK);
  if (nprobe < 1) return fail(PROQA_EINVAL, "ivf_search: nprobe=%d < 1", nprobe);
  if (dtype != PROQA_F16 && dtype != PROQA_F32) return fail(PROQA_EINVAL, "ivf_search: dtype=%d", dtype);
  if (!h->trained) return fail(PROQA_EINVAL, "ivf_search: the index is not trained");
  if (nq < 0 || nq >= (1ll << 31) / kIvfMaxProbe) return fail(PROQA_EINVAL, "ivf_search: nq=%lld", (long long)nq);
  const int np = std::min(nprobe, h->nlist);
  if (np > kIvfMaxProbe) return fail(PROQA_EINVAL, "ivf_search: min(nprobe, nlist)=%d above %d", np, kIvfMaxProbe);
  if (nq == 0) return PROQA_OK;
  if (!xq_dev || !D_dev || !I_dev) return fail(PROQA_EINVAL, "ivf_search: NULL argument");
  PROQA_ON_DEVICE(h->device);
  hipStream_t st = as_stream(stream);
  const int nlist = h->nlist;
  int rc;
  if ((rc = ensure(h->w_xq, (size_t)nq * kDim * 2)) || (rc = ensure(h->w_probes, (size_t)nq * np * sizeof(int))) ||
      (rc = ensure(h->w_rank, (size_t)nq * np * sizeof(int))) || (rc = ensure(h->w_qn2, (size_t)nq * sizeof(float))) ||
      (rc = ensure(h->w_counts, ((size_t)nlist + 2) * sizeof(unsigned))) ||
      (rc = ensure(h->w_bucket, (size_t)nq * np * sizeof(int))))
    return rc;
  PROQA_HIP(hipEventRecord(h->ev[0], st));
  unsigned* counts = (unsigned*)h->w_counts.p;   // [nlist] query counts, [nlist, nlist + 2) the conversion flags
  PROQA_HIP(hipMemsetAsync(counts, 0, ((size_t)nlist + 2) * sizeof(unsigned), st));
  const void* xq16 = xq_dev;
  if (dtype == PROQA_F32) {
    PROQA_HIP(launch_convert_f32_to_f16((const float*)xq_dev, h->w_xq.p, nq * kDim, counts + nlist, st));
    xq16 = h->w_xq.p;
  }
  int* probes = (int*)h->w_probes.p;
  int* rank = (int*)h->w_rank.p;
  float* qn2 = (float*)h->w_qn2.p;
  PROQA_HIP(launch_ivf_coarse(xq16, nq, h->cent, nlist, np, probes, rank, qn2, counts, st));
  // the one host round trip of a search: how many queries probe each list
  PROQA_HIP(hipMemcpyAsync(h->counts_host, counts, ((size_t)nlist + 2) * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  PROQA_HIP(hipStreamSynchronize(st));
  if (h->counts_host[nlist + 1]) return fail(PROQA_EINVAL, "ivf_search: float32 queries beyond the fp16 range");
  if (h->counts_host[nlist] && !h->allow_rounding)
    return fail(PROQA_EINVAL, "ivf_search: float32 queries that fp16 cannot hold (allow_rounding rounds them)");
  // work items: (list, chunk of its rows, tile of 32 of its queries); chunks shrink until the launch fills the GPU
  long long pair_rows = 0, tiles_rows = 0;
  for (int l = 0; l < nlist; ++l) {
    const long long size = h->off[l + 1] - h->off[l];
    pair_rows += size * h->counts_host[l];
    tiles_rows += size * ceil_div<long long>(h->counts_host[l], kIvfTileQ);
  }
  long long chunk = 32768;
  const long long want_items = 4ll * device_cu_count();
  while (chunk > 4096 && tiles_rows / chunk < want_items) chunk /= 2;
  const size_t tbl_ints = ((size_t)nlist + 1) + nlist;    // qoff, nch
  const size_t tbl_bytes = round_up<size_t>(tbl_ints * sizeof(int), 16) + (size_t)nlist * sizeof(long long);
  h->table.assign(tbl_bytes, 0);
  int* qoff = (int*)h->table.data();
  int* nch = qoff + nlist + 1;
  long long* slot0 = (long long*)(h->table.data() + round_up<size_t>(tbl_ints * sizeof(int), 16));
  h->work.clear();
  long long slots = 0;
  int qacc = 0;
  for (int l = 0; l < nlist; ++l) {
    const long long size = h->off[l + 1] - h->off[l];
    const int cq = (int)h->counts_host[l];
    qoff[l] = qacc;
    nch[l] = cq && size ? (int)ceil_div<long long>(size, chunk) : 0;
    slot0[l] = slots;
    slots += (long long)cq * nch[l];
    qacc += cq;
    for (int c = 0; c < nch[l]; ++c)
      for (int t = 0; t < ceil_div(cq, kIvfTileQ); ++t) {
        const long long r0 = h->off[l] + c * chunk;
        h->work.push_back(IvfWork{l, c, t, 0, r0, std::min(r0 + chunk, h->off[l + 1])});
      }
  }
  qoff[nlist] = qacc;
  if (h->work.size() >= (1u << 31)) return fail(PROQA_EINVAL, "ivf_search: too many work items");
  if ((rc = ensure(h->w_table, tbl_bytes)) || (rc = ensure(h->w_work, std::max<size_t>(1, h->work.size()) * sizeof(IvfWork))) ||
      (rc = ensure(h->w_partial, std::max<long long>(1, slots) * (size_t)k * sizeof(unsigned long long))))
    return rc;
  PROQA_HIP(hipMemcpyAsync(h->w_table.p, h->table.data(), tbl_bytes, hipMemcpyHostToDevice, st));
  if (!h->work.empty())
    PROQA_HIP(hipMemcpyAsync(h->w_work.p, h->work.data(), h->work.size() * sizeof(IvfWork), hipMemcpyHostToDevice, st));
  IvfListTable lt;
  lt.qoff = (const int*)h->w_table.p;
  lt.nch = lt.qoff + nlist + 1;
  lt.slot0 = (const long long*)((const char*)h->w_table.p + round_up<size_t>(tbl_ints * sizeof(int), 16));
  int* bucket = (int*)h->w_bucket.p;
  unsigned long long* partial = (unsigned long long*)h->w_partial.p;
  PROQA_HIP(launch_ivf_bucket(probes, rank, nq, np, lt.qoff, bucket, st));
  PROQA_HIP(hipEventRecord(h->ev[1], st));
  PROQA_HIP(launch_ivf_scan(h->xs, h->hn, h->ids, xq16, bucket, lt, (const IvfWork*)h->w_work.p, (int)h->work.size(), k,
                            partial, st));
  PROQA_HIP(hipEventRecord(h->ev[2], st));
  PROQA_HIP(launch_ivf_merge(partial, probes, rank, nq, np, lt, k, h->xs, h->pos, xq16, qn2, D_dev, (long long*)I_dev, ip_dev,
                             st));
  PROQA_HIP(hipEventRecord(h->ev[3], st));
  h->stats = proqa_ivf_stats{};
  h->stats.nq = nq;
  h->stats.rows_scanned = pair_rows;
  h->stats.nprobe = np;
  h->stats.work_items = (int32_t)h->work.size();
  h->stats.chunk_rows = (int32_t)chunk;
  h->stats.partial_lists = slots;
  h->stats_pending = true;
  return PROQA_OK;
}

int proqa_ivf_search_stats(proqa_ivf* h, proqa_ivf_stats* out) {
  if (!h || !out) return fail(PROQA_EINVAL, "ivf_search_stats: NULL argument");
  if (h->stats_pending) {
    PROQA_ON_DEVICE(h->device);
    PROQA_HIP(hipEventSynchronize(h->ev[3]));
    PROQA_HIP(hipEventElapsedTime(&h->stats.search_ms, h->ev[0], h->ev[3]));
    PROQA_HIP(hipEventElapsedTime(&h->stats.scan_ms, h->ev[1], h->ev[2]));
    h->stats_pending = false;
  }
  *out = h->stats;
  return PROQA_OK;
}

int proqa_ivf_reconstruct_batch_device(const proqa_ivf* h, const int64_t* ids_dev, int64_t n, void* out_dev, int out_dtype,
                                       void* stream) {
  if (!h || (n > 0 && (!ids_dev || !out_dev))) return fail(PROQA_EINVAL, "ivf_reconstruct: NULL argument");
  if (out_dtype != PROQA_F16 && out_dtype != PROQA_F32) return fail(PROQA_EINVAL, "ivf_reconstruct: out_dtype=%d", out_dtype);
  if (n <= 0) return PROQA_OK;
  PROQA_ON_DEVICE(h->device);
  PROQA_HIP(launch_ivf_gather(h->xs, h->pos, h->ntotal, (const long long*)ids_dev, n, out_dev, out_dtype == PROQA_F32,
                              as_stream(stream)));
  return PROQA_OK;
}

}  // extern "C"
