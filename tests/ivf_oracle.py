"""NumPy restatement of faiss 1.6.3 IndexIVFFlat(IndexFlatIP quantizer, d, nlist) -- TEST INFRASTRUCTURE ONLY.

The reference builds it at qa/online_sampler.py:75-79 (no metric argument: METRIC_L2) and searches it at :274.  faiss is
not installed here, so its source behaviour is restated:
  train   Level1Quantizer: Clustering(d, nlist), niter 10, max_points_per_centroid 256, seed 1234, assignment by the
          quantizer's inner product (oracle.kmeans_oracle.train(x, nlist, 10, 256, l2=False))
  add     every row to the list of its largest inner product with the centroids, ties to the lowest list, input order
  search  the nprobe lists of largest inner product (correctly rounded fp32 scores, ties to the lowest list), then the k
          rows of smallest sum (q - x)^2 among them, ties to the lowest id; the tail of a short result is I = -1,
          D = +FLT_MAX.
Distances are exact (float64, rounded once to float32).
"""
import numpy as np

from oracle import kmeans_oracle

FLT_MAX = np.float32(3.4028234663852886e38)


def train(x, nlist):
    """float32 centroids [nlist, d]"""
    cent, _ = kmeans_oracle.train(x, nlist, 10, 256, l2=False)
    return cent


def assign(x, centroids):
    """list of every row (int64 [n])"""
    return kmeans_oracle.assign(x, centroids, l2=False)[1]


def lists(assignment, nlist):
    """ids of every list in list order (= ascending id)"""
    return [np.nonzero(assignment == l)[0] for l in range(nlist)]


def coarse(xq, centroids, nprobe):
    """int64 [nq, min(nprobe, nlist)]: the probed lists, best first"""
    s = (np.asarray(xq, np.float32).astype(np.float64) @ np.asarray(centroids, np.float32).astype(np.float64).T).astype(np.float32)
    nlist = s.shape[1]
    order = np.lexsort((np.broadcast_to(np.arange(nlist), s.shape), -s.astype(np.float64)), axis=1)
    return order[:, :min(nprobe, nlist)]


def search(xq, xb, assignment, centroids, nprobe, k):
    """(D float32 [nq, k], I int64 [nq, k])"""
    xq64 = np.asarray(xq, np.float32).astype(np.float64)
    xb64 = np.asarray(xb, np.float32).astype(np.float64)
    nlist = centroids.shape[0]
    members = lists(assignment, nlist)
    probes = coarse(xq, centroids, nprobe)
    nq = xq64.shape[0]
    D = np.full((nq, k), FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        cand = np.concatenate([members[l] for l in probes[q]]) if probes.shape[1] else np.zeros(0, np.int64)
        if cand.size == 0:
            continue
        d = ((xb64[cand] - xq64[q]) ** 2).sum(1)
        order = np.lexsort((cand, d))[:k]
        D[q, :order.size] = d[order].astype(np.float32)
        I[q, :order.size] = cand[order]
    return D, I


def brute_l2(xq, xb, k):
    """exact L2 top-k over all rows (ties to the lowest id)"""
    xq64 = np.asarray(xq, np.float32).astype(np.float64)
    xb64 = np.asarray(xb, np.float32).astype(np.float64)
    nq = xq64.shape[0]
    D = np.full((nq, k), FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    ids = np.arange(xb64.shape[0])
    for q in range(nq):
        d = ((xb64 - xq64[q]) ** 2).sum(1)
        order = np.lexsort((ids, d))[:k]
        D[q, :order.size] = d[order].astype(np.float32)
        I[q, :order.size] = order
    return D, I
