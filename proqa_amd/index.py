"""Exact inner-product index on MI355X, with the call shape of faiss.IndexFlatIP.

The reference searches with

    index = faiss.IndexFlatIP(d); index.add(xb); D, I = index.search(xq, k)

(/root/reference/retrieval/eval_retrieval.py:102-104, also retrieval/trec_process.py:74-76).
`IndexFlatIP` here keeps that shape (numpy in, numpy out) over libproqa_hip.so;
`ShardedIndexFlatIP` row-shards the corpus over the ranks of a torch.distributed group (one
process per GPU, RCCL over xGMI), all-gathers the per-shard (score, id) lists once and merges
them on the GPU.  `IndexIVFFlat` is the reference's other index, faiss.IndexIVFFlat(IndexFlatIP quantizer, d, nlist)
with its default L2 metric (qa/online_sampler.py:75-79).  None of the classes has a CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import PROQA_F16, PROQA_F32, EMBED_DIM


def _np_dtype_code(arr):
    if arr.dtype == np.float16:
        return PROQA_F16
    if arr.dtype == np.float32:
        return PROQA_F32
    raise TypeError(f"embeddings must be float16 or float32, got {arr.dtype}")


def _torch_dtype_code(t):
    import torch
    if t.dtype == torch.float16:
        return PROQA_F16
    if t.dtype == torch.float32:
        return PROQA_F32
    raise TypeError(f"embeddings must be float16 or float32, got {t.dtype}")


def _as_matrix(x, d, what):
    x = np.ascontiguousarray(x)
    if x.ndim != 2 or x.shape[1] != d:
        raise ValueError(f"{what} must have shape [n, {d}], got {x.shape}")
    return x


QUERY_BATCH = 16384   # queries per library call: bounds the per-search candidate store in HBM


class IndexFlatIP:
    """Brute-force maximum-inner-product index; rows live in HBM as fp16."""

    def __init__(self, d=EMBED_DIM, capacity=0):
        self._lib = _lib.load()
        _lib.require_gpu()
        self.d = int(d)
        handle = ctypes.c_void_p()
        _lib.check(self._lib.proqa_index_create(self.d, int(capacity), ctypes.byref(handle)))
        self._h = handle
        self._adopted = None  # keeps an adopted tensor alive

    # -- faiss-shaped API ---------------------------------------------------------------
    @property
    def ntotal(self):
        n = ctypes.c_int64()
        _lib.check(self._lib.proqa_index_ntotal(self._h, ctypes.byref(n)))
        return n.value

    def add(self, xb):
        """Append rows.  numpy [n,d] float16/float32 (host) or a CUDA torch tensor."""
        if _is_torch(xb):
            return self.add_device(xb)
        xb = _as_matrix(xb, self.d, "xb")
        _lib.check(self._lib.proqa_index_add(self._h, xb.ctypes.data, xb.shape[0], _np_dtype_code(xb)))

    def add_npy(self, path, row0=0, n=-1, readers=0):
        """np.load(path)[row0:row0+n] + add, streamed by the library (reader threads -> pinned ring -> HBM; n < 0: to the
        last row).  The file's dtype ('<f2' / '<f4') follows the precision rules of add()."""
        _lib.check(self._lib.proqa_index_add_npy(self._h, str(path).encode(), int(row0), int(n), int(readers)))

    def search(self, xq, k):
        """(D float32 [nq,k], I int64 [nq,k]); scores descending, ties by ascending row."""
        if _is_torch(xq):
            D, I = self.search_device(xq, k)
            return D.cpu().numpy(), I.cpu().numpy()
        xq = _as_matrix(xq, self.d, "xq")
        nq = xq.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        for q0 in range(0, max(nq, 1), QUERY_BATCH):
            part = xq[q0:q0 + QUERY_BATCH]
            _lib.check(self._lib.proqa_index_search(self._h, part.ctypes.data, part.shape[0], _np_dtype_code(xq),
                                                    int(k), D[q0:].ctypes.data, I[q0:].ctypes.data))
        return D, I

    def reset(self):
        _lib.check(self._lib.proqa_index_reset(self._h))
        self._adopted = None

    # -- device-resident variants -------------------------------------------------------
    def add_device(self, xb):
        import torch
        if not xb.is_cuda:
            raise ValueError("add_device expects a CUDA tensor")
        xb = xb.contiguous()
        if xb.dim() != 2 or xb.shape[1] != self.d:
            raise ValueError(f"xb must have shape [n, {self.d}], got {tuple(xb.shape)}")
        with torch.cuda.device(xb.device):
            _lib.check(self._lib.proqa_index_add_device(self._h, xb.data_ptr(), xb.shape[0], _torch_dtype_code(xb),
                                                        _lib.current_stream_ptr()))

    def adopt_device(self, xb):
        """Search caller-owned fp16 rows in place (no copy); the tensor is kept alive here.

        The rows must not change while adopted: searches of k <= 128 over >= 65536 rows scan an int8 copy of them
        (+128 B per row) that is built once.  After writing into the tensor call `rows_changed()` -- or switch the copy
        off with `configure_nomination("off")`; otherwise results can silently miss rows."""
        import torch
        if not (xb.is_cuda and xb.dtype == torch.float16 and xb.is_contiguous() and xb.dim() == 2
                and xb.shape[1] == self.d):
            raise ValueError("adopt_device expects a contiguous CUDA float16 [n, d] tensor")
        torch.cuda.current_stream().synchronize()
        _lib.check(self._lib.proqa_index_adopt_device(self._h, xb.data_ptr(), xb.shape[0]))
        self._adopted = xb

    def rows_changed(self):
        """The adopted tensor was modified in place: the int8 copy of the rows is rebuilt before its next use."""
        _lib.check(self._lib.proqa_index_rows_changed(self._h))

    def prepare(self):
        """Build now what the first search would otherwise build (the int8 copy of the rows: 128 B per row, ~3 ms per
        18M rows, one host wait).  Optional; `search` / `search_device` build it on demand, the enqueued search of
        ShardedIndexFlatIP leaves it to the end of its first step."""
        import torch
        _lib.check(self._lib.proqa_index_prepare(self._h, _lib.current_stream_ptr() if torch.cuda.is_available() else None))

    def search_device(self, xq, k, idx_offset=0, out=None):
        """CUDA tensor in, CUDA tensors out: (D float32 [nq,k], I int64 [nq,k]); `out` = (D, I) to write into."""
        import torch
        if not xq.is_cuda:
            raise ValueError("search_device expects a CUDA tensor")
        xq = xq.contiguous()
        if xq.dim() != 2 or xq.shape[1] != self.d:
            raise ValueError(f"xq must have shape [nq, {self.d}], got {tuple(xq.shape)}")
        nq = xq.shape[0]
        if out is not None:
            D, I = out
            if (tuple(D.shape), D.dtype, tuple(I.shape), I.dtype) != ((nq, k), torch.float32, (nq, k), torch.int64) or \
                    not (D.is_contiguous() and I.is_contiguous() and D.device == xq.device and I.device == xq.device):
                raise ValueError("out must be contiguous (float32 [nq,k], int64 [nq,k]) tensors on xq's device")
        else:
            D = torch.empty((nq, k), dtype=torch.float32, device=xq.device)
            I = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
        with torch.cuda.device(xq.device):
            for q0 in range(0, max(nq, 1), QUERY_BATCH):
                part = xq[q0:q0 + QUERY_BATCH]
                _lib.check(self._lib.proqa_index_search_device(self._h, part.data_ptr(), part.shape[0],
                                                               _torch_dtype_code(xq), int(k), int(idx_offset),
                                                               D[q0:].data_ptr(), I[q0:].data_ptr(),
                                                               _lib.current_stream_ptr()))
        return D, I

    def reconstruct_batch_device(self, ids, dtype=None, idx_offset=0):
        """Rows of the index by id (faiss reconstruct_batch) without leaving the GPU: ids int64 CUDA tensor of any shape
        (e.g. the I of search_device) -> [*ids.shape, d] tensor of `dtype` (torch.float16, the stored rows, or
        torch.float32); ids outside the index (-1 of a short result) give zero rows."""
        import torch
        if not ids.is_cuda or ids.dtype != torch.int64:
            raise ValueError("reconstruct_batch_device expects an int64 CUDA tensor")
        dtype = dtype or torch.float16
        ids = ids.contiguous()
        out = torch.empty(tuple(ids.shape) + (self.d,), dtype=dtype, device=ids.device)
        with torch.cuda.device(ids.device):
            _lib.check(self._lib.proqa_index_reconstruct_batch_device(self._h, ids.data_ptr(), ids.numel(), int(idx_offset),
                                                                      out.data_ptr(), _torch_dtype_code(out),
                                                                      _lib.current_stream_ptr()))
        return out

    def collect_labeled_device(self, ids, gold_rows, head, dtype=None, idx_offset=0):
        """The collect step of the reference's online sampler (qa/online_sampler.py:117-136) in one launch: ids int64 CUDA
        tensor [k] (a row of search_device's I), gold_rows int64 CUDA tensor of strictly ascending ids (or None) ->
        (rows [k, d] as reconstruct_batch_device gives them, labels int32 [k]: 1 where the id is a row of the index and
        occurs in gold_rows, record int64 [2 + head]: the number of ids that are rows of the index, the sum of the
        labels, ids[:head] padded with -1).  Nothing leaves the GPU."""
        import torch
        if not ids.is_cuda or ids.dtype != torch.int64:
            raise ValueError("collect_labeled_device expects an int64 CUDA tensor")
        if gold_rows is not None and (not gold_rows.is_cuda or gold_rows.dtype != torch.int64 or gold_rows.dim() != 1):
            raise ValueError("collect_labeled_device expects gold_rows as a 1-D int64 CUDA tensor")
        if ids.dim() != 1:
            raise ValueError(f"ids must have shape [k], got {tuple(ids.shape)}")
        head = int(head)            # outside [0, 64]: the library's PROQA_EINVAL
        dtype = dtype or torch.float16
        ids = ids.contiguous()
        k = ids.numel()
        n_gold = 0 if gold_rows is None else gold_rows.numel()
        gold_rows = gold_rows.contiguous() if n_gold else None
        rows = torch.empty((k, self.d), dtype=dtype, device=ids.device)
        labels = torch.empty((k,), dtype=torch.int32, device=ids.device)
        record = torch.empty((2 + min(max(head, 0), 64),), dtype=torch.int64, device=ids.device)
        with torch.cuda.device(ids.device):
            _lib.check(self._lib.proqa_sampler_collect_device(
                self._h, ids.data_ptr() if k else None, k, int(idx_offset), gold_rows.data_ptr() if n_gold else None, n_gold,
                head, rows.data_ptr() if k else None, _torch_dtype_code(rows), labels.data_ptr() if k else None,
                record.data_ptr(), _lib.current_stream_ptr()))
        return rows, labels, record

    def collect_labeled_multi_device(self, ids, gold_rows, gold_begin, gold_count, head, dtype=None, idx_offset=0):
        """collect_labeled_device for the Q rows of one search_device result, in one launch: ids int64 CUDA tensor [Q, k],
        gold_rows the int64 CUDA buffer that holds every question's list (or None), gold_begin / gold_count: Q host
        integers each, question q's list being gold_rows[gold_begin[q] : gold_begin[q] + gold_count[q]] (strictly
        ascending; empty lists, shared lists are legal) -> (rows [Q, k, d], labels int32 [Q, k], records int64
        [Q, 2 + head]), row q of each being what collect_labeled_device returns for ids[q] and that list.  The bounds go
        to the kernel by value: nothing is copied to or from the GPU."""
        import torch
        if not ids.is_cuda or ids.dtype != torch.int64:
            raise ValueError("collect_labeled_multi_device expects an int64 CUDA tensor")
        if gold_rows is not None and (not gold_rows.is_cuda or gold_rows.dtype != torch.int64 or gold_rows.dim() != 1):
            raise ValueError("collect_labeled_multi_device expects gold_rows as a 1-D int64 CUDA tensor")
        if ids.dim() != 2:
            raise ValueError(f"ids must have shape [Q, k], got {tuple(ids.shape)}")
        nq, k = ids.shape
        begin, count = [int(b) for b in gold_begin], [int(c) for c in gold_count]
        if len(begin) != nq or len(count) != nq:
            raise ValueError(f"gold_begin and gold_count must hold one entry per question ({nq}), got {len(begin)} and {len(count)}")
        head = int(head)            # outside [0, 64]: the library's PROQA_EINVAL
        dtype = dtype or torch.float16
        ids = ids.contiguous()
        n_gold = 0 if gold_rows is None else gold_rows.numel()
        gold_rows = gold_rows.contiguous() if n_gold else None
        rows = torch.empty((nq, k, self.d), dtype=dtype, device=ids.device)
        labels = torch.empty((nq, k), dtype=torch.int32, device=ids.device)
        records = torch.empty((nq, 2 + min(max(head, 0), 64)), dtype=torch.int64, device=ids.device)
        some = nq * k > 0
        with torch.cuda.device(ids.device):
            _lib.check(self._lib.proqa_sampler_collect_multi_device(
                self._h, ids.data_ptr() if some else None, nq, k, int(idx_offset), gold_rows.data_ptr() if n_gold else None,
                n_gold, (ctypes.c_int64 * nq)(*begin), (ctypes.c_int64 * nq)(*count), head,
                rows.data_ptr() if some else None, _torch_dtype_code(rows), labels.data_ptr() if some else None,
                records.data_ptr() if nq else None, _lib.current_stream_ptr()))
        return rows, labels, records

    # -- introspection / tuning ---------------------------------------------------------
    def last_stats(self):
        st = _lib.SearchStats()
        _lib.check(self._lib.proqa_index_last_stats(self._h, ctypes.byref(st)))
        return {"rounds": st.rounds, "fallback_rounds": st.fallback_rounds, "candidates": st.candidates,
                "filter_ms": st.filter_ms, "total_ms": st.total_ms, "nominated": st.nominated,
                "nomination": bool(st.nomination),
                "nomination_state": ("off", "on", "suspended")[st.nomination_state] if 0 <= st.nomination_state <= 2 else None,
                "leap_rank": st.leap_rank,
                "leap_state": ("off", "on", "paused")[st.leap_state] if 0 <= st.leap_state <= 2 else None}

    def set_profiling(self, enable=True):
        _lib.check(self._lib.proqa_index_set_profiling(self._h, 1 if enable else 0))

    @property
    def exact_f32(self):
        """True once a float32 row or query that fp16 cannot hold has switched the index to
        exact-float32 mode (float32 copies of the rows, fp16 scan + exact re-scoring)."""
        v = ctypes.c_int(0)
        _lib.check(self._lib.proqa_index_is_exact_f32(self._h, ctypes.byref(v)))
        return bool(v.value)

    def allow_rounding(self, allow=True):
        """Round float32 inputs to fp16 instead of switching to exact-float32 mode (faster merge, half
        the memory; results are then those of the rounded vectors).  Off by default: the reference
        searches float32."""
        _lib.check(self._lib.proqa_index_allow_rounding(self._h, 1 if allow else 0))

    def configure(self, first_slab_rows=0, growth=0):
        """Round schedule: rows of the first (dense) slab and the growth factor of later slabs."""
        _lib.check(self._lib.proqa_index_configure(self._h, first_slab_rows, growth))

    def configure_bootstrap(self, rows):
        """Rows covered by the dense bootstrap (exact top-k of the first rows from a score matrix); 0 disables it."""
        _lib.check(self._lib.proqa_index_configure_bootstrap(self._h, int(rows)))

    def configure_nomination(self, mode):
        """The int8 nomination scan of the k <= 128 rounds (see proqa_hip.h): 0 / "off" = fp16 scan only, 1 / "auto"
        (default: a search that over-nominates suspends the int8 rounds, later searches re-probe them; `last_stats()
        ["nomination_state"]`, one stderr line per switch under PROQA_LOG=1), 2 / "always".  The result is the fp16
        scan's either way."""
        mode = {"off": 0, "auto": 1, "always": 2}.get(mode, mode)
        _lib.check(self._lib.proqa_index_configure_nomination(self._h, int(mode)))

    def configure_leap(self, mode):
        """Leaping rounds of the k <= 128 searches (see proqa_hip.h): thresholds at a rank j < k of the running lists, a
        third to a half of the rounds; a round that falls short is re-scanned (the result never depends on it) and pauses
        the leaps of this index (`last_stats()["leap_rank"]`, `["leap_state"]`).  0 / "off", 1 / "auto" (default)."""
        mode = {"off": 0, "auto": 1}.get(mode, mode)
        _lib.check(self._lib.proqa_index_configure_leap(self._h, int(mode)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.proqa_index_free(self._h)
            self._h = None
            self._adopted = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _is_torch(x):
    return type(x).__module__.startswith("torch")


METRIC_INNER_PRODUCT = 0   # faiss' metric constants; IndexIVFFlat offers METRIC_L2 only
METRIC_L2 = 1
IVF_MAX_K = 128            # kIvfMaxK of the library
IVF_QUERY_BATCH = 4096     # queries per library call: bounds the partial lists of a search in HBM


class IndexIVFFlat:
    """faiss.IndexIVFFlat(quantizer, d, nlist) as the reference's qa/online_sampler.py:75-79 builds it, on MI355X.

    faiss 1.6.3 semantics, restated (faiss is not installed here; nothing below is pinned against it):
      - the metric is L2: `IndexIVFFlat(quantizer, d, nlist)` without a metric argument is METRIC_L2 (faiss source).  The
        quantizer, an IndexFlatIP, picks the probed lists by INNER PRODUCT; inside them rows rank by squared L2 distance
        (D ascending).  Rows of large norm win by inner product and lose by L2: the result is not an approximation of
        the exact inner-product top k.
      - train(x): Level1Quantizer's training, Clustering(d, nlist) with niter = 10 (the value Level1Quantizer sets),
        max_points_per_centroid = 256, seed 1234, assignment by the quantizer's inner product = group_paras.KMeans(...,
        spherical_metric=True).  The centroids end up in the quantizer (quantizer.ntotal == nlist).
      - add(x): every row to the list of its largest inner product with the centroids (ties to the lowest list), after
        the list's earlier rows, ids ntotal + i.
      - search(xq, k): the nprobe lists of largest inner product (ties to the lowest list; probes past nlist are skipped),
        then the k rows of smallest sum (q - x)^2 among them; exact distance ties go to the lowest id (faiss leaves it
        unspecified).  Fewer than k probed rows: the tail is I = -1, D = +FLT_MAX (the L2 heap's neutral value).
      - faiss computes the coarse scores in fp32 (sgemm, or its own loops below 20 queries); here they are correctly
        rounded (double accumulation), so the two can probe different lists only where two centroid scores lie within
        fp32 round-off of each other.
    Rows and queries are fp16, or float32 that fp16 holds exactly (the --fp16 .npy payload, the fp16 question tower);
    other float32 input is refused unless allow_rounding(True).  1 <= k <= 128.  No CPU path."""

    def __init__(self, quantizer, d=EMBED_DIM, nlist=100, metric=METRIC_L2):
        if not isinstance(quantizer, IndexFlatIP):
            raise TypeError(f"IndexIVFFlat: the quantizer must be a proqa_amd.index.IndexFlatIP, got {type(quantizer).__name__}")
        if metric != METRIC_L2:
            raise ValueError("IndexIVFFlat: only METRIC_L2 (faiss' default) is offered")
        if quantizer.d != int(d):
            raise ValueError(f"IndexIVFFlat: quantizer.d={quantizer.d}, d={d}")
        if quantizer.ntotal:
            raise ValueError("IndexIVFFlat: the quantizer must be empty (train() puts the centroids into it)")
        self._lib = _lib.load()
        _lib.require_gpu()
        self.quantizer = quantizer
        self.d = int(d)
        self.nlist = int(nlist)
        self.nprobe = 1
        self._rounding = False
        self.centroids = None
        handle = ctypes.c_void_p()
        _lib.check(self._lib.proqa_ivf_create(self.d, self.nlist, ctypes.byref(handle)))
        self._h = handle

    # -- inputs ---------------------------------------------------------------------------
    def _device(self):
        import torch
        return torch.device("cuda", torch.cuda.current_device())

    def _rows_f16(self, x, what):
        """CUDA fp16 [n, d] tensor of x (numpy or torch); float32 must be held exactly by fp16 unless allow_rounding."""
        import torch
        if not _is_torch(x):
            x = _as_matrix(x, self.d, what)
            if x.dtype not in (np.float16, np.float32):
                raise TypeError(f"{what} must be float16 or float32, got {x.dtype}")
            dev = self._device()
            out = torch.empty((x.shape[0], self.d), dtype=torch.float16, device=dev)
            step = 1 << 21
            for r0 in range(0, x.shape[0], step):
                out[r0:r0 + step] = self._to_f16(torch.from_numpy(x[r0:r0 + step]).to(dev), what)
            return out
        if not x.is_cuda:
            x = x.to(self._device())
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"{what} must have shape [n, {self.d}], got {tuple(x.shape)}")
        return self._to_f16(x, what).contiguous()

    def _to_f16(self, t, what):
        import torch
        if t.dtype == torch.float16:
            return t
        if t.dtype != torch.float32:
            raise TypeError(f"{what} must be float16 or float32, got {t.dtype}")
        h = t.half()
        if not self._rounding and not torch.equal(h.float(), t):
            raise ValueError(f"{what}: float32 values that fp16 cannot hold (allow_rounding(True) rounds them)")
        return h

    # -- faiss-shaped API ---------------------------------------------------------------
    @property
    def is_trained(self):
        return self.centroids is not None

    @property
    def ntotal(self):
        n = ctypes.c_int64()
        _lib.check(self._lib.proqa_ivf_ntotal(self._h, ctypes.byref(n)))
        return n.value

    def allow_rounding(self, allow=True):
        """Round float32 rows and queries that fp16 cannot hold instead of refusing them (off by default)."""
        self._rounding = bool(allow)
        _lib.check(self._lib.proqa_ivf_allow_rounding(self._h, 1 if allow else 0))

    def train(self, x):
        from .group_paras import KMeans
        if self.ntotal:
            raise RuntimeError("IndexIVFFlat.train: the index holds rows (reset() first)")
        x16 = self._rows_f16(x, "x")
        import torch
        with torch.cuda.device(x16.device):
            km = KMeans(self.d, self.nlist, niter=10, max_points_per_centroid=256, seed=1234, spherical_metric=True)
            km.train(x16)
            self.set_centroids(km.centroids)

    def add(self, x):
        if not self.is_trained:
            raise RuntimeError("IndexIVFFlat.add: train() first")
        x16 = self._rows_f16(x, "x")
        import torch
        with torch.cuda.device(x16.device):
            _lib.check(self._lib.proqa_ivf_add_device(self._h, x16.data_ptr(), x16.shape[0], _lib.current_stream_ptr()))

    def _check_search(self, k):
        k = int(k)
        if not 1 <= k <= IVF_MAX_K:
            raise ValueError(f"IndexIVFFlat.search: k={k}; this index searches 1 <= k <= {IVF_MAX_K} "
                             "(IndexFlatIP searches any k)")
        if int(self.nprobe) < 1:
            raise ValueError(f"IndexIVFFlat.search: nprobe={self.nprobe} < 1")
        return k

    def search(self, xq, k, inner_products=False):
        """(D float32 [nq,k], I int64 [nq,k]) as numpy arrays (+ the inner products q.x when inner_products)."""
        k = self._check_search(k)
        if not _is_torch(xq):
            xq = _as_matrix(xq, self.d, "xq")
            _np_dtype_code(xq)
            import torch
            xq = torch.from_numpy(xq).to(self._device())
        out = self.search_device(xq, k, inner_products=inner_products)
        return tuple(t.cpu().numpy() for t in out)

    def search_device(self, xq, k, inner_products=False):
        """CUDA tensor in, CUDA tensors out: (D, I) or, with inner_products, (D, I, IP) -- IP [nq,k] float32 has the bits
        IndexFlatIP reports for the same (query, row)."""
        import torch
        k = self._check_search(k)
        if not self.is_trained:
            raise RuntimeError("IndexIVFFlat.search: train() first")
        if not xq.is_cuda:
            raise ValueError("search_device expects a CUDA tensor")
        xq = xq.contiguous()
        if xq.dim() != 2 or xq.shape[1] != self.d:
            raise ValueError(f"xq must have shape [nq, {self.d}], got {tuple(xq.shape)}")
        code = _torch_dtype_code(xq)
        nq = xq.shape[0]
        D = torch.empty((nq, k), dtype=torch.float32, device=xq.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
        IP = torch.empty((nq, k), dtype=torch.float32, device=xq.device) if inner_products else None
        self._batch_stats = []       # the library's statistics of the earlier calls of this search (last_stats sums them)
        with torch.cuda.device(xq.device):
            for q0 in range(0, max(nq, 1), IVF_QUERY_BATCH):
                if q0:
                    self._batch_stats.append(self._library_stats())   # (waits for the previous call's kernels)
                part = xq[q0:q0 + IVF_QUERY_BATCH]
                _lib.check(self._lib.proqa_ivf_search_device(self._h, part.data_ptr(), code, part.shape[0], k, int(self.nprobe),
                                                             D[q0:].data_ptr(), I[q0:].data_ptr(),
                                                             IP[q0:].data_ptr() if IP is not None else None,
                                                             _lib.current_stream_ptr()))
        return (D, I, IP) if inner_products else (D, I)

    def reconstruct_batch_device(self, ids, dtype=None):
        """Rows by original id (as IndexFlatIP.reconstruct_batch_device): ids int64 CUDA tensor of any shape ->
        [*ids.shape, d] of `dtype` (torch.float16 or torch.float32); ids outside the index give zero rows."""
        import torch
        if not ids.is_cuda or ids.dtype != torch.int64:
            raise ValueError("reconstruct_batch_device expects an int64 CUDA tensor")
        dtype = dtype or torch.float16
        ids = ids.contiguous()
        out = torch.empty(tuple(ids.shape) + (self.d,), dtype=dtype, device=ids.device)
        with torch.cuda.device(ids.device):
            _lib.check(self._lib.proqa_ivf_reconstruct_batch_device(self._h, ids.data_ptr(), ids.numel(), out.data_ptr(),
                                                                    _torch_dtype_code(out), _lib.current_stream_ptr()))
        return out

    def list_sizes(self):
        sizes = np.zeros(self.nlist, dtype=np.int64)
        _lib.check(self._lib.proqa_ivf_list_sizes(self._h, sizes.ctypes.data))
        return sizes

    def list_ids(self):
        """[ids of list l in list order for l in range(nlist)] (numpy int64 arrays)"""
        ids = np.zeros(self.ntotal, dtype=np.int64)
        _lib.check(self._lib.proqa_ivf_list_ids(self._h, ids.ctypes.data))
        return np.split(ids, np.cumsum(self.list_sizes())[:-1])

    def set_centroids(self, centroids):
        """Use these float32 centroids [nlist, d] instead of training (they go into the quantizer too); only while the
        index holds no rows."""
        import torch
        cent = torch.as_tensor(centroids, dtype=torch.float32)
        cent = (cent if cent.is_cuda else cent.to(self._device())).contiguous()
        if tuple(cent.shape) != (self.nlist, self.d):
            raise ValueError(f"centroids must have shape [{self.nlist}, {self.d}], got {tuple(cent.shape)}")
        with torch.cuda.device(cent.device):
            _lib.check(self._lib.proqa_ivf_set_centroids(self._h, cent.data_ptr()))
            self.quantizer.reset()
            self.quantizer.add_device(cent)
        self.centroids = cent

    def _library_stats(self):
        st = _lib.IvfStats()
        _lib.check(self._lib.proqa_ivf_search_stats(self._h, ctypes.byref(st)))
        return st

    def last_stats(self):
        """Of the last search, summed over its library calls (IVF_QUERY_BATCH queries each): queries, rows scanned (the
        sum over the queries of their probed list sizes) and per query, lists probed per query, partial lists, scan work
        items, the rows per chunk of the last call, and the HIP-event times (ms) of the searches and of their scans.  A
        search that failed reports zeros."""
        parts = list(getattr(self, "_batch_stats", [])) + [self._library_stats()]
        nq = sum(p.nq for p in parts)
        rows = sum(p.rows_scanned for p in parts)
        return {"nq": nq, "rows_scanned": rows, "rows_scanned_per_query": rows / nq if nq else 0.0,
                "lists_probed": parts[-1].nprobe, "partial_lists": sum(p.partial_lists for p in parts),
                "work_items": sum(p.work_items for p in parts), "chunk_rows": parts[-1].chunk_rows,
                "search_ms": sum(p.search_ms for p in parts), "scan_ms": sum(p.scan_ms for p in parts),
                "library_calls": len(parts)}

    def reset(self):
        """Drop the rows (the centroids stay, as in faiss)."""
        _lib.check(self._lib.proqa_ivf_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.proqa_ivf_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PipelinedSearcher:
    """A STREAM of query batches over one set of rows, two searches in flight.

    One search is a chain of ~20 dependent launches (bootstrap, rounds of scan + merge, finalize) and a host wait; at the
    shard sizes of a multi-GPU job the chain is a third of the step.  Two IndexFlatIP handles over the same adopted rows,
    each on its own stream, take the batches in turn: batch i+1 is enqueued (proqa_index_search_begin_device) before the
    host waits for batch i (proqa_index_search_finish), so one search's small launches run beside the other's large
    scans.  Results are those of the one-call search, in order.  Cost: every handle builds its own int8 copy of the rows
    (+128 B per row each) and its own workspace.  Measured: 1.08 x the call-by-call rate at 18M rows, 1.19 x at 2.25M
    (2032 queries, k = 80; profiles/ABLATIONS.md R6.3).  The reference searches once (eval_retrieval.py:102-104); this is
    for callers that have many batches (an evaluation loop over several query files, the online sampler)."""

    def __init__(self, xb, d=EMBED_DIM):
        import torch
        self.handles = [IndexFlatIP(d), IndexFlatIP(d)]
        self.streams = [torch.cuda.Stream(device=xb.device), torch.cuda.Stream(device=xb.device)]
        for h in self.handles:
            h.adopt_device(xb)
            h.prepare()
        self.d = d

    def search_batches(self, batches, k, idx_offset=0):
        """Generator: for every CUDA tensor [nq, d] of `batches` one (D float32 [nq,k], I int64 [nq,k]), in order; a batch's
        result is complete (host-synchronised) when it is yielded."""
        import torch
        lib = _lib.load()
        k = int(k)
        pending = []
        try:
            for n, xq in enumerate(batches):
                slot = n & 1
                if len(pending) == 2:
                    yield self._finish(pending.pop(0))
                if not xq.is_cuda or xq.dim() != 2 or xq.shape[1] != self.d:
                    raise ValueError(f"batches must be CUDA tensors of shape [nq, {self.d}]")
                if xq.shape[0] > QUERY_BATCH:
                    raise ValueError(f"at most {QUERY_BATCH} queries per batch")
                xq = xq.contiguous()
                nq = xq.shape[0]
                D = torch.empty((nq, k), dtype=torch.float32, device=xq.device)
                I = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
                st = self.streams[slot]
                st.wait_stream(torch.cuda.current_stream(xq.device))  # the batch may still be on its way on the caller's stream
                with torch.cuda.device(xq.device):
                    _lib.check(lib.proqa_index_search_begin_device(self.handles[slot]._h, xq.data_ptr(), nq, _torch_dtype_code(xq),
                                                                   k, int(idx_offset), D.data_ptr(), I.data_ptr(), None,
                                                                   st.cuda_stream))
                pending.append((slot, xq, D, I))
            while pending:
                yield self._finish(pending.pop(0))
        finally:
            # a consumer that stops early (or an error above): the searches still in flight write into tensors this frame
            # is about to drop -- complete them first
            for item in pending:
                try:
                    self._finish(item)
                except Exception:
                    pass

    def _finish(self, item):
        slot, _xq, D, I = item
        _lib.check(_lib.load().proqa_index_search_finish(self.handles[slot]._h, None))
        return D, I

    def last_stats(self):
        return [h.last_stats() for h in self.handles]

    def close(self):
        for h in self.handles:
            h.close()


def merge_topk_device(D_parts, I_parts):
    """Merge [n_parts, nq, k] per-shard lists (ascending shard order) into [nq, k] on the GPU.  The parts need not be
    sorted inside (this entry point sorts); slots with I = -1 are missing rows wherever they sit."""
    import torch
    lib = _lib.load()
    D_parts = D_parts.contiguous()
    I_parts = I_parts.contiguous()
    n_parts, nq, k = D_parts.shape
    D = torch.empty((nq, k), dtype=torch.float32, device=D_parts.device)
    I = torch.empty((nq, k), dtype=torch.int64, device=D_parts.device)
    with torch.cuda.device(D_parts.device):
        _lib.check(lib.proqa_topk_merge_device(D_parts.data_ptr(), I_parts.data_ptr(), n_parts, nq, k,
                                               D.data_ptr(), I.data_ptr(), _lib.current_stream_ptr()))
    return D, I


def shard_bounds(n_rows, world_size, rank):
    """Contiguous row range of `rank`: rows [r*N/G, (r+1)*N/G)."""
    lo = (n_rows * rank) // world_size
    hi = (n_rows * (rank + 1)) // world_size
    return lo, hi


class QueryShardedIndexFlatIP:
    """The other decomposition of the multi-GPU search: every rank holds ALL rows, the QUERIES are sharded.

    An 18M x 128 fp16 index and its int8 copy are 6.9 GB of a GPU's 288 GB.  Rank r searches queries [r nq / G, (r + 1) nq / G)
    over the whole corpus (IndexFlatIP, i.e. the HBM-bound small-batch regime for the usual 2032 queries on 8 ranks) and the
    ranks all-gather their result rows: no rank merge, nothing to exchange but the answer, and every query's result is the
    single-GPU search's by construction.  Measured on one GPU: 254 queries over 18M rows 0.72 ms, against 0.81-0.83 ms for
    2032 queries over a 2.25M-row shard before its all-gather and merge (`bench.py --gpus N` reports
    this decomposition as `query_shards` beside the row-sharded `value` that BASELINE configs[3] prescribes).
    `local_search(xq, k) -> (D, I)` is injectable so that the plumbing runs under gloo on CPU in the tests."""

    def __init__(self, d=EMBED_DIM, group=None, local_search=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.world_size = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.d = d
        self._local_search = local_search
        self._index = IndexFlatIP(d) if local_search is None else None

    @property
    def local_index(self):
        return self._index

    def add(self, xb):
        """ALL rows of the corpus, on every rank (host array or CUDA tensor)."""
        self._index.add(xb)

    def add_npy(self, path, readers=0):
        """every rank loads the whole .npy index file"""
        self._index.add_npy(path, 0, -1, readers)

    def adopt(self, xb):
        """search all rows in place (a contiguous CUDA fp16 tensor, see IndexFlatIP.adopt_device)"""
        self._index.adopt_device(xb)

    def prepare(self):
        if self._index is not None:
            self._index.prepare()

    def search(self, xq, k):
        """All ranks call with the same queries [nq, d]; returns (D float32 [nq,k], I int64 [nq,k]) on xq's device, on every
        rank.  ONE collective: the ranks' result rows (ids and scores as one byte buffer per rank, padded to equal slices)."""
        import torch
        nq = xq.shape[0]
        per = (nq + self.world_size - 1) // self.world_size
        q0, q1 = min(self.rank * per, nq), min((self.rank + 1) * per, nq)
        mine = xq[q0:q1].contiguous()
        if q1 > q0:
            D, I = self._local_search(mine, k) if self._local_search is not None else self._index.search_device(mine, k)
        else:
            D = torch.empty((0, k), dtype=torch.float32, device=xq.device)
            I = torch.empty((0, k), dtype=torch.int64, device=xq.device)
        if self.world_size == 1:
            return D, I
        Dp = torch.zeros((per, k), dtype=torch.float32, device=D.device)
        Ip = torch.full((per, k), -1, dtype=torch.int64, device=D.device)
        Dp[:q1 - q0] = D
        Ip[:q1 - q0] = I
        n_i, n_d = Ip.numel() * 8, Dp.numel() * 4
        block = torch.cat([Ip.view(torch.uint8).reshape(-1), Dp.view(torch.uint8).reshape(-1)])
        gathered = torch.empty((self.world_size, n_i + n_d), dtype=torch.uint8, device=D.device)
        if self.dist.get_backend(self.group) == "nccl":     # RCCL
            self.dist.all_gather_into_tensor(gathered, block, group=self.group)
        elif gathered.is_cuda:                               # gloo with two ranks on one GPU (tests): staged through the host
            parts = [torch.empty_like(block, device="cpu") for _ in range(self.world_size)]
            self.dist.all_gather(parts, block.cpu(), group=self.group)
            gathered = torch.stack(parts).to(D.device)
        else:
            self.dist.all_gather(list(gathered.unbind(0)), block, group=self.group)
        I_all = gathered[:, :n_i].contiguous().view(torch.int64).reshape(self.world_size * per, k)
        D_all = gathered[:, n_i:].contiguous().view(torch.float32).reshape(self.world_size * per, k)
        return D_all[:nq].contiguous(), I_all[:nq].contiguous()

    def close(self):
        if self._index is not None:
            self._index.close()
            self._index = None


class ShardedIndexFlatIP:
    """Row-sharded exact index over a torch.distributed process group (one rank per GPU).

    Every rank holds rows [lo, hi) of the corpus and all queries; `search` runs the local exact
    top-k with global row ids, all-gathers the [nq, k] (score, id) lists of every rank (the only
    collective on the path) and merges them with the same ordering rule, so the result is
    bit-identical to the single-GPU search.  `local_search` / `merge` are injectable so the
    distributed plumbing can be exercised with the gloo backend on CPU in the tests.
    """

    def __init__(self, n_total, d=EMBED_DIM, group=None, local_search=None, merge=None, preallocate=True,
                 transport="torch"):
        """transport: who runs the all-gather -- "torch" (torch.distributed, RCCL under the nccl backend) or "cabi"
        (libproqa_hip.so's own RCCL communicator, proqa_sharded_search_device: the path a caller without PyTorch
        uses; torch.distributed only carries the 128-byte communicator id to the ranks here)."""
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.world_size = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.n_total = int(n_total)
        self.d = d
        self.lo, self.hi = shard_bounds(self.n_total, self.world_size, self.rank)
        self._local_search = local_search
        self._merge = merge or merge_topk_device
        self._index = None
        self._comm = None
        if transport not in ("torch", "cabi"):
            raise ValueError(f"unknown transport {transport!r}")
        self.transport = transport
        if local_search is None:
            self._index = IndexFlatIP(d, capacity=(self.hi - self.lo) if preallocate else 0)
        if transport == "cabi":
            if self._index is None:
                raise ValueError('transport="cabi" needs the built-in HIP searcher')
            self._comm = self._create_comm()

    def _create_comm(self):
        """proqa_comm over the ranks of the group: rank 0 draws the id, every rank joins (a collective)."""
        lib = _lib.load()
        ident = ctypes.create_string_buffer(128)
        if self.rank == 0:
            _lib.check(lib.proqa_comm_get_unique_id(ident))
        if self.world_size > 1:
            box = [ident.raw]
            self.dist.broadcast_object_list(box, src=self.dist.get_global_rank(self.group, 0) if self.group else 0,
                                            group=self.group)
            ident = ctypes.create_string_buffer(box[0], 128)
        handle = ctypes.c_void_p()
        _lib.check(lib.proqa_comm_create(ident, self.world_size, self.rank, ctypes.byref(handle)))
        return handle

    def add_local(self, xb_local):
        """Add this rank's rows (exactly rows [lo, hi) of the corpus, in order)."""
        if self._index is None:
            raise RuntimeError("add_local is only available with the built-in HIP searcher")
        self._index.add(xb_local)
        if self._index.ntotal > self.hi - self.lo:
            raise ValueError("more rows added than this rank's shard holds")

    def add_local_npy(self, path, readers=0):
        """Load this rank's rows [lo, hi) of the .npy index file straight into HBM (every rank reads only its range)."""
        if self._index is None:
            raise RuntimeError("add_local_npy is only available with the built-in HIP searcher")
        if self._index.ntotal:
            raise ValueError("this rank's shard already holds rows")
        self._index.add_npy(path, self.lo, self.hi - self.lo, readers)

    def adopt_local(self, xb_local):
        """Search this rank's rows [lo, hi) in place: a contiguous CUDA fp16 tensor, not copied (and not to be modified
        while adopted: see IndexFlatIP.adopt_device / rows_changed)."""
        if self._index is None:
            raise RuntimeError("adopt_local is only available with the built-in HIP searcher")
        if xb_local.shape[0] != self.hi - self.lo:
            raise ValueError(f"rank {self.rank} holds rows [{self.lo}, {self.hi}), got {xb_local.shape[0]} rows")
        self._index.adopt_device(xb_local)

    def prepare(self):
        """Every rank builds the int8 copy of its shard now (IndexFlatIP.prepare) instead of at the end of its first
        search step."""
        if self._index is not None:
            self._index.prepare()

    @property
    def local_index(self):
        return self._index

    def search(self, xq, k, force_collective=False):
        """All ranks call with the same queries; returns torch tensors (D, I) on xq's device.
        force_collective: go through the all-gather and the merge even with a single rank."""
        import torch
        if self._comm is not None:
            return self._search_cabi(xq, k)
        exchange = self.world_size > 1 or force_collective
        if exchange and not self.dist.is_initialized():
            raise RuntimeError('force_collective with transport="torch" needs an initialised torch.distributed process '
                               'group (transport="cabi" brings its own RCCL communicator)')
        if exchange and self._local_search is None and self._merge is merge_topk_device and \
                self.dist.get_backend(self.group) == "nccl":
            return self._search_in_place(xq, k)
        if self._local_search is not None:
            D, I = self._local_search(xq, k, self.lo)
        else:
            D, I = self._index.search_device(xq, k, idx_offset=self.lo)
        if not exchange:
            return D, I
        # ONE collective: ids (int64) and scores (float32) travel as one byte buffer per rank;
        # rank-ordered slices of the gathered buffer are exactly the [n_parts, nq, k] layout the merge consumes
        n_i, n_d = I.numel() * 8, D.numel() * 4
        mine = torch.cat([I.contiguous().view(torch.uint8).reshape(-1), D.contiguous().view(torch.uint8).reshape(-1)])
        gathered = torch.empty((self.world_size, n_i + n_d), dtype=torch.uint8, device=D.device)
        if self.dist.get_backend(self.group) == "nccl":     # RCCL: one flat collective, no staging copies
            self.dist.all_gather_into_tensor(gathered, mine, group=self.group)
        else:                                                # gloo (CPU tests, two ranks on one GPU)
            self.dist.all_gather(list(gathered.unbind(0)), mine, group=self.group)
        I_all = gathered[:, :n_i].contiguous().view(torch.int64).reshape((self.world_size,) + tuple(I.shape))
        D_all = gathered[:, n_i:].contiguous().view(torch.float32).reshape((self.world_size,) + tuple(D.shape))
        return self._merge(D_all, I_all)

    def _search_in_place(self, xq, k):
        """The RCCL exchange without staging copies and without a host round trip in the middle: the local search is
        only ENQUEUED (proqa_index_search_begin_device) and writes its ids and scores straight into this rank's block
        [ids | scores | status word, 16 B] of the send buffer; ONE all_gather_into_tensor and the strided merge
        (proqa_topk_merge_strided_device), which reads the receive buffer where it lies, go onto the stream right behind
        it; the host waits once, at the end (proqa_index_search_finish).  The status words of all ranks come back with
        the blocks: a rank whose candidate lists overflowed (status 1) rewrites its list in _finish and every rank runs
        the exchange once more; a rank whose local search failed (status 0xFFFFFFFF) still enters the collective, and
        every rank raises instead of waiting for it."""
        import torch
        if not xq.is_cuda:
            raise ValueError("sharded search expects a CUDA tensor")
        xq = xq.contiguous()
        if xq.dim() != 2 or xq.shape[1] != self.d:
            raise ValueError(f"xq must have shape [nq, {self.d}], got {tuple(xq.shape)}")
        k = int(k)
        if k <= 0:
            raise ValueError(f"k={k}")
        nq = xq.shape[0]
        D_out = torch.empty((nq, k), dtype=torch.float32, device=xq.device)
        I_out = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
        # (every rank sees the same nq: with no query nobody enters the collective; above QUERY_BATCH queries the search
        # runs slice by slice like IndexFlatIP.search_device -- the candidate store of the library grows with nq)
        for q0 in range(0, nq, QUERY_BATCH):
            self._exchange_slice(xq[q0:q0 + QUERY_BATCH], k, D_out[q0:q0 + QUERY_BATCH], I_out[q0:q0 + QUERY_BATCH])
        return D_out, I_out

    def _exchange_slice(self, xq, k, D_out, I_out):
        """begin -> all-gather -> strided merge -> finish for one slice of at most QUERY_BATCH queries; D_out / I_out are
        contiguous [nq, k] views that receive the merged result."""
        import torch
        lib = _lib.load()
        nq = xq.shape[0]
        sizes = [ctypes.c_size_t() for _ in range(3)]
        _lib.check(lib.proqa_sharded_block_layout(nq, k, *[ctypes.byref(v) for v in sizes]))
        n_i, n_d, block = (v.value for v in sizes)
        # the send / receive buffers are kept from call to call (one set per slice size: the full slice and the tail)
        key = (nq, k, xq.device)
        cache = self.__dict__.setdefault("_xchg", {})
        if key not in cache:
            if len(cache) >= 2:
                cache.clear()
            cache[key] = (torch.empty(block, dtype=torch.uint8, device=xq.device),
                          torch.empty((self.world_size, block), dtype=torch.uint8, device=xq.device),
                          torch.zeros(self.world_size, dtype=torch.int32).pin_memory())
        mine, gathered, status_host = cache[key]
        status_dev = mine.data_ptr() + n_i + n_d
        failure = None
        with torch.cuda.device(xq.device):
            try:
                _lib.check(lib.proqa_index_search_begin_device(self._index._h, xq.data_ptr(), nq, _torch_dtype_code(xq), k,
                                                               int(self.lo), mine.data_ptr() + n_i, mine.data_ptr(), status_dev,
                                                               _lib.current_stream_ptr()))
            except Exception as e:       # still enter the collective: the other ranks are already on their way into it
                failure = e
            for _attempt in range(2):
                if failure is not None:
                    mine[n_i + n_d:n_i + n_d + 4] = 0xFF
                self.dist.all_gather_into_tensor(gathered, mine, group=self.group)
                # (the merge kernel drops every rank's status word into the pinned host buffer: no copy on the stream)
                _lib.check(lib.proqa_topk_merge_gathered_device(gathered.data_ptr(), self.world_size, nq, k,
                                                                status_host.data_ptr(), D_out.data_ptr(), I_out.data_ptr(),
                                                                _lib.current_stream_ptr()))
                if failure is None:
                    try:
                        _lib.check(lib.proqa_index_search_finish(self._index._h, None))
                    except Exception as e:
                        failure = e
                torch.cuda.current_stream().synchronize()
                status = status_host.tolist()
                if -1 in status:
                    raise failure if failure is not None else RuntimeError(
                        f"sharded search: rank {status.index(-1)} failed in its local search")
                if not any(status):
                    if failure is not None:     # the lists were exchanged (nobody waits), but this rank's result may be incomplete
                        raise failure
                    return
                if failure is None:
                    mine[n_i + n_d:n_i + n_d + 4] = 0
        raise RuntimeError("sharded search: the ranks did not agree on a final result")

    def _search_cabi(self, xq, k):
        """proqa_sharded_search_device: local search, RCCL all-gather and merge inside the library."""
        import torch
        if not xq.is_cuda:
            raise ValueError("sharded search expects a CUDA tensor")
        xq = xq.contiguous()
        nq = xq.shape[0]
        D = torch.empty((nq, k), dtype=torch.float32, device=xq.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
        lib = _lib.load()
        with torch.cuda.device(xq.device):
            for q0 in range(0, max(nq, 1), QUERY_BATCH):
                part = xq[q0:q0 + QUERY_BATCH]
                _lib.check(lib.proqa_sharded_search_device(self._index._h, self._comm, part.data_ptr(), part.shape[0],
                                                           _torch_dtype_code(xq), int(k), int(self.lo),
                                                           D[q0:].data_ptr(), I[q0:].data_ptr(),
                                                           _lib.current_stream_ptr()))
        return D, I

    def close(self):
        if getattr(self, "_comm", None):
            _lib.load().proqa_comm_free(self._comm)
            self._comm = None
        if getattr(self, "_index", None) is not None:
            self._index.close()
            self._index = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
