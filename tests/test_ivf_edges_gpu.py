"""IndexIVFFlat at the edges of its scan, merge and coarse kernels, against tests/ivf_oracle.py.

Integer worlds (every score exact in fp32; tests/test_ivf_host.py asserts it, and that each world has the shape it claims):
I, D and the inner products are compared bit for bit, no tolerance.  Worlds of fp16 rows that are not integers: the bound
on D derived in ivf_oracle's header, D >= 0, and set membership within that bound.  Every index gets its centroids from
set_centroids: nothing here trains."""
import numpy as np
import pytest
import torch

import ivf_oracle

pytestmark = pytest.mark.gpu

WORLDS = ivf_oracle.integer_worlds()


def _index(cent, x, device):
    from proqa_amd.index import IndexFlatIP, IndexIVFFlat
    index = IndexIVFFlat(IndexFlatIP(128), 128, len(cent))
    index.set_centroids(torch.from_numpy(np.ascontiguousarray(cent, np.float32)).to(device))
    index.add(torch.from_numpy(x).to(device))
    return index


def _search(index, xq, k, device):
    return tuple(t.cpu().numpy() for t in index.search_device(torch.from_numpy(xq).to(device), k, inner_products=True))


def _check_exact(index, xq, x, Do, Io, k, device):
    """the search of xq equals the oracle's (Do, Io: at least k columns) bit for bit; IP is the float64 inner product"""
    D, I, IP = _search(index, xq, k, device)
    np.testing.assert_array_equal(I, Io[:len(xq), :k])
    np.testing.assert_array_equal(D, Do[:len(xq), :k])
    live = I >= 0
    with np.errstate(invalid="ignore"):
        ip_o = np.einsum("qd,qkd->qk", xq.astype(np.float64), x[np.maximum(I, 0)].astype(np.float64))
    np.testing.assert_array_equal(IP[live], ip_o[live].astype(np.float32))
    assert (IP[~live] == -ivf_oracle.FLT_MAX).all()


def _lists_follow_the_oracle(index, a, nlist):
    want = ivf_oracle.lists(a, nlist)
    got = index.list_ids()
    assert len(got) == nlist
    for l in range(nlist):
        np.testing.assert_array_equal(got[l], want[l])


# 1. one list, exact row counts: the tile of 32, the step of 4 x 32, the 256-key lists, the 4096-row chunk
@pytest.mark.parametrize("n", ivf_oracle.LINE_ROWS)
@pytest.mark.parametrize("order", ivf_oracle.LINE_ORDERS)
def test_one_list_at_exact_row_counts(gpu_device, order, n):
    x, cent, xq = WORLDS[f"line-{order}-{n}"][0]()
    a = np.zeros(n, np.int64)
    Do, Io = ivf_oracle.search(xq, x, a, cent, 1, 128)
    index = _index(cent, x, gpu_device)
    assert index.list_sizes().tolist() == [n]
    for k in ivf_oracle.LINE_KS:
        for nq in ivf_oracle.LINE_NQS:
            _check_exact(index, xq[:nq], x, Do, Io, k, gpu_device)
            st = index.last_stats()
            chunks = -(-n // 4096)
            assert st["chunk_rows"] == 4096 and st["work_items"] == chunks * -(-nq // 32)
            assert st["partial_lists"] == nq * chunks and st["rows_scanned"] == nq * n


def test_one_list_with_a_tied_score_across_two_cuts(gpu_device):
    """ivf_oracle.plateau_profile: keys left out of a full list that tie with the new k-th score at lower ids"""
    x, cent, xq = WORLDS["line-plateau-640"][0]()
    Do, Io = ivf_oracle.search(xq, x, np.zeros(640, np.int64), cent, 1, 128)
    assert (np.sort(Io, axis=1) == np.concatenate([np.arange(384, 494), np.arange(512, 530)])).all()
    index = _index(cent, x, gpu_device)
    for k in (128, 80, 5):
        _check_exact(index, xq, x, Do, Io, k, gpu_device)


# 2. several chunks and several query tiles
@pytest.mark.parametrize("world", ["chunks-ascending", "chunks-descending", "chunks-random", "chunks-edges"])
def test_three_chunks_and_three_query_tiles(gpu_device, world):
    x, cent, xq = WORLDS[world][0]()
    assert len(x) == 9000 and len(xq) == 70
    a = np.zeros(9000, np.int64)
    Do, Io = ivf_oracle.search(xq, x, a, cent, 1, 128)
    if world == "chunks-ascending":
        assert (Io >= 8192).all()                  # every winner in the last chunk
    if world == "chunks-descending":
        assert (Io < 4096).all()                   # ... in the first
    if world == "chunks-edges":
        assert set(Io[:, 0]) == set(ivf_oracle.CHUNK_EDGE_ROWS)
    index = _index(cent, x, gpu_device)
    for k in (1, 80, 128):
        _check_exact(index, xq, x, Do, Io, k, gpu_device)
        st = index.last_stats()
        assert st["chunk_rows"] == 4096 and st["work_items"] == 9 and st["partial_lists"] == 70 * 3


# 3a. merge batches: 64 partial lists per query, 31 per batch at k = 128, 50 at k = 80, all in one at k = 1
@pytest.mark.parametrize("winners", ["last", "first"])
def test_merge_batches_with_the_winners_probed_last_or_first(gpu_device, winners):
    x, cent, xq = ivf_oracle.merge_world(winners)
    a = ivf_oracle.assign(x, cent)
    index = _index(cent, x, gpu_device)
    _lists_follow_the_oracle(index, a, 64)
    index.nprobe = 64
    Do, Io = ivf_oracle.search(xq, x, a, cent, 64, 128)
    for k in (128, 80, 1):
        _check_exact(index, xq, x, Do, Io, k, gpu_device)
        st = index.last_stats()
        assert st["partial_lists"] == 40 * 64 and st["lists_probed"] == 64 and st["rows_scanned"] == 40 * len(x)


# 3b. nlist 4096 (the whole LDS key array of the coarse step), 1024 probes (the whole prefix table of the merge)
def test_4096_lists_1024_probes_and_the_refusal_above(gpu_device):
    from proqa_amd._lib import ProqaError
    x, cent, xq = ivf_oracle.sign_world()
    a = ivf_oracle.assign(x, cent)
    index = _index(cent, x, gpu_device)
    _lists_follow_the_oracle(index, a, 4096)
    sizes = index.list_sizes()
    probes = ivf_oracle.coarse(xq, cent, 1024)
    assert (sizes > 0).sum() >= 1024 and (sizes[probes] > 0).all(1).any() and (sizes[probes] == 0).any()
    Do, Io = ivf_oracle.search(xq, x, a, cent, 1024, 128)
    for k in (5, 128):
        index.nprobe = 5000                        # min(nprobe, nlist) = 4096 > 1024: refused
        with pytest.raises(ProqaError, match="4096 above 1024"):
            index.search_device(torch.from_numpy(xq).to(gpu_device), k)
        assert index.last_stats()["nq"] == 0
        index.nprobe = 1024
        _check_exact(index, xq, x, Do, Io, k, gpu_device)
        st = index.last_stats()
        assert st["lists_probed"] == 1024 and st["rows_scanned"] == int(sizes[probes].sum())
        assert st["partial_lists"] == int((sizes[probes] > 0).sum())


# 4. the coarse step: nlist 1 (two sort keys), no power of two (padding keys), duplicated, zero and all-negative centroids
@pytest.mark.parametrize("nlist", ivf_oracle.COARSE_NLISTS)
def test_coarse_step_at_small_and_odd_list_counts(gpu_device, nlist):
    x, cent, xq = ivf_oracle.coarse_world(nlist)
    a = ivf_oracle.assign(x, cent)
    index = _index(cent, x, gpu_device)
    _lists_follow_the_oracle(index, a, nlist)
    sizes = index.list_sizes()
    for nprobe in (1, nlist, nlist + 5):
        index.nprobe = nprobe
        Do, Io = ivf_oracle.search(xq, x, a, cent, nprobe, 128)
        probes = ivf_oracle.coarse(xq, cent, nprobe)
        for k in (5, 128):
            _check_exact(index, xq, x, Do, Io, k, gpu_device)
            st = index.last_stats()
            assert st["lists_probed"] == min(nprobe, nlist) and st["rows_scanned"] == int(sizes[probes].sum())


# 5. fp16 rows that are not integers: the derived bound on D, D >= 0, membership within the bound
@pytest.mark.parametrize("world", ivf_oracle.FLOAT_WORLDS)
def test_distances_of_float_rows_keep_the_derived_bound_and_are_not_negative(gpu_device, world):
    x, cent, xq = ivf_oracle.float_world(world)
    index = _index(cent, x, gpu_device)
    a = np.empty(len(x), np.int64)                 # the index's lists (integer worlds pin the assignment itself)
    for l, ids in enumerate(index.list_ids()):
        a[ids] = l
    assert (a != ivf_oracle.assign(x, cent)).sum() <= 2
    index.nprobe = 3
    x64, q64 = x.astype(np.float64), xq.astype(np.float64)
    probes = ivf_oracle.coarse(xq, cent, 3)
    for k in (5, 128):
        D, I, IP = _search(index, xq, k, gpu_device)
        _, Io = ivf_oracle.search(xq, x, a, cent, 3, k)
        assert (I >= 0).all() and (Io >= 0).all()
        worst = 0.0
        for q in range(len(xq)):
            assert len(set(I[q])) == k and np.isin(a[I[q]], probes[q]).all()
            exact = ((x64[I[q]] - q64[q]) ** 2).sum(1)
            bound = ivf_oracle.distance_bound(xq[q], x[I[q]])
            err = np.abs(D[q].astype(np.float64) - exact)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (q, float((err / bound).max()))
            kth = x[Io[q, -1:]]
            d_k = float(((kth.astype(np.float64) - q64[q]) ** 2).sum())
            b_k = float(ivf_oracle.distance_bound(xq[q], kth)[0])
            assert (exact <= d_k + b_k).all(), q                                          # nothing returned from far below
            missing = np.setdiff1d(Io[q], I[q])
            assert (((x64[missing] - q64[q]) ** 2).sum(1) >= d_k - b_k).all(), q          # nothing near left out
            assert (np.abs(IP[q] - x64[I[q]] @ q64[q]) <= ivf_oracle.GAMMA * ivf_oracle.U * (np.abs(x64[I[q]]) @ np.abs(q64[q]))).all(), q
        print(f"{world} k={k}: min D {D.min():.3e}, negative D {(D < 0).sum()} of {D.size}, worst |D - D*| / bound {worst:.3f}")
        assert (np.diff(D, axis=1) >= 0).all()
        assert (D >= 0).all(), (int((D < 0).sum()), float(D.min()))


# 6. rows holding +-inf or NaN: add takes them, a search never returns them (faiss' heap takes d < FLT_MAX only)
def test_non_finite_rows_are_never_returned(gpu_device):
    x, cent, xq = ivf_oracle.nonfinite_world()
    index = _index(cent, x, gpu_device)
    assert index.ntotal == 223
    a = np.empty(223, np.int64)
    for l, ids in enumerate(index.list_ids()):
        a[ids] = l
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(a, ivf_oracle.assign(x, cent))
    assert (a[220:] == 0).all()                    # +inf with centroid 0 and -inf with the others, or NaN with all: list 0
    for nprobe in (1, 4):
        index.nprobe = nprobe
        Do, Io = ivf_oracle.search(xq, x, a, cent, nprobe, 80)
        Df, If = ivf_oracle.search(xq, x[:220], a[:220], cent, nprobe, 80)
        np.testing.assert_array_equal(Io, If)      # the oracle's result is that of the finite rows alone
        np.testing.assert_array_equal(Do, Df)
        _check_exact(index, xq, x, Do, Io, 80, gpu_device)
        D, I, IP = _search(index, xq, 80, gpu_device)
        if nprobe == 1:                            # queries 0..7 probe list 0: its 40 finite rows, then the tail
            assert (np.sort(I[:8, :40], axis=1) == np.arange(40)).all()
            assert (I[:8, 40:] == -1).all() and (D[:8, 40:] == ivf_oracle.FLT_MAX).all()
            assert (IP[:8, 40:] == -ivf_oracle.FLT_MAX).all()
        assert index.last_stats()["rows_scanned"] == int(np.bincount(a, minlength=4)[ivf_oracle.coarse(xq, cent, nprobe)].sum())
