"""The last step of the row-sharded search with MORE THAN ONE part, in one process on one GPU.

RCCL refuses two ranks on one device, so the suite's RCCL runs (test_rccl_gpu.py) merge exactly one part, and the
multi-part merges elsewhere (merge_topk_device, the gloo ranks of test_distributed_gpu.py) take the SORTING kernels by
design.  What only `n_parts >= 2` switches on is covered here:

  A. proqa_topk_merge_gathered_device (merge_sorted_lists, the rank merge: no sort, a binary search per part) on
     synthetic receive buffers -- against a NumPy lexsort of the union, against the sorting merge on the same buffer
     (an independent kernel), and the per-part status words it drops into pinned host memory; every branch of
     launch_merge_lists that can carry status words.
  B. an N-rank sharded search with real searches: N handles enqueue (proqa_index_search_begin_device) into their
     blocks of one [N, block] buffer -- what the all-gather would deliver --, one merge, the finishes, one
     synchronisation, the status words, a second merge if a word says so: the sequence of proqa_sharded_search_device
     with the collective replaced by shared memory.
  C. ShardedIndexFlatIP._search_in_place as rank r of a world of 8, with a stub in place of torch.distributed whose
     all-gather delivers prepared peer blocks: the multi-rank branches of the exchange protocol (a peer asks for a
     second exchange, a peer is poisoned, the ranks never agree).

Every comparison is exact (ids equal, score bits equal).  Nothing here initialises RCCL or starts a process."""
import ctypes
import functools
import zlib

import numpy as np
import pytest

from oracle import search_oracle

pytestmark = pytest.mark.gpu

NEG_FILL = search_oracle.NEG_FILL
POISON_D = 0x7FC0DEAD                    # a NaN: never a score of these tests
POISON_I = 0x5A5A5A5A5A5A5A5A
POISON_STATUS = 0x5EED                   # what the pinned status words hold before the kernel writes them
K_POISON = 0xFFFFFFFF                    # "that rank failed"


def _layout(nq, k):
    """(ids bytes, scores bytes, block bytes) of a per-rank block, from the library: the status word's place depends on it"""
    from proqa_amd import _lib
    sizes = [ctypes.c_size_t() for _ in range(3)]
    _lib.check(_lib.load().proqa_sharded_block_layout(nq, k, *[ctypes.byref(v) for v in sizes]))
    return tuple(v.value for v in sizes)


def _pack_blocks(Dp, Ip, words):
    """[n_parts, block] bytes as the all-gather leaves them: per part [ids int64 nq*k | scores f32 nq*k | status word];
    every byte the layout pads with is 0xA5"""
    n_parts, nq, k = Dp.shape
    n_i, n_d, block = _layout(nq, k)
    buf = np.full((n_parts, block), 0xA5, np.uint8)
    for p in range(n_parts):
        buf[p, :nq * k * 8] = np.ascontiguousarray(Ip[p], np.int64).view(np.uint8).reshape(-1)
        buf[p, n_i:n_i + nq * k * 4] = np.ascontiguousarray(Dp[p], np.float32).view(np.uint8).reshape(-1)
        buf[p, n_i + n_d:n_i + n_d + 4] = np.frombuffer(np.uint32(words[p]).tobytes(), np.uint8)
    return buf


def _poisoned_out(nq, k, device):
    import torch
    D = torch.empty((max(nq, 1), k), dtype=torch.float32, device=device)     # (nq = 0: the entry point wants a pointer)
    I = torch.empty((max(nq, 1), k), dtype=torch.int64, device=device)
    D.view(torch.int32).fill_(POISON_D)
    I.fill_(POISON_I)
    return D, I


def _pinned_status(n_parts):
    import torch
    return torch.full((n_parts,), POISON_STATUS, dtype=torch.int32).pin_memory()


def _merge_gathered(g, n_parts, nq, k, status_host, device):
    """proqa_topk_merge_gathered_device into poisoned outputs"""
    from proqa_amd import _lib
    D, I = _poisoned_out(nq, k, device)
    _lib.check(_lib.load().proqa_topk_merge_gathered_device(g.data_ptr(), n_parts, nq, k,
                                                            status_host.data_ptr() if status_host is not None else None,
                                                            D.data_ptr(), I.data_ptr(), _lib.current_stream_ptr()))
    return D, I


def _u32(words):
    return [w & 0xFFFFFFFF for w in words]


# ---- A. the merge entry point on synthetic gathered buffers --------------------------------------------------------------

def _status_words(n_parts):
    return [(0, 1, K_POISON)[p] if p < 3 else p + 2 for p in range(n_parts)]


def _make_parts(rng, n_parts, nq, k, scores, counts):
    """Per-part lists as a search reports them: scores descending, equal scores by ascending id (+0.0 and -0.0 are equal),
    I = -1 / D = -FLT_MAX only at the tail, ids ascending with the part index (gathered position order == global id order) and
    beyond 2^32."""
    shape = (n_parts, nq, k)
    stride = k + k // 2 + 3
    ids = np.sort(np.argsort(rng.random((n_parts, nq, stride)), axis=2)[:, :, :k], axis=2).astype(np.int64)
    ids += (np.arange(n_parts, dtype=np.int64) * stride)[:, None, None] + (1 << 33)
    if scores == "zeros":
        S = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], np.float32), shape)
    else:   # ~7 integer values: many ties that cross parts, the k-th boundary regularly inside a tie group
        S = rng.integers(-3, 4, shape).astype(np.float32)
    if scores == "inf":   # +inf at the head of every other part
        for p in range(0, n_parts, 2):
            S[p, :, :1 + p % 3] = np.inf
    if counts == "full":
        c = np.full((n_parts, nq), k)
    elif counts == "short":
        c = rng.choice(np.array([0, 1, k // 2, k - 1, k]), (n_parts, nq))
    elif counts == "short_total":   # all parts together hold fewer than k rows: the tail fill starts at n_valid > 0
        assert k > 1
        c = rng.multinomial(max(1, k // 3), np.full(n_parts, 1.0 / n_parts), nq).T
    elif counts == "all_empty":
        c = np.zeros((n_parts, nq), np.int64)
    else:   # "disagree": a query whose parts are all full beside a query whose parts are all empty
        assert counts == "disagree"
        c = np.where(np.arange(nq) % 2 == 0, k, 0)[None, :].repeat(n_parts, 0)
    valid = np.arange(k)[None, None, :] < c[:, :, None]
    order = np.lexsort((ids, np.where(valid, -S.astype(np.float64), np.inf)), axis=2)
    Dp = np.where(valid, np.take_along_axis(S, order, axis=2), NEG_FILL).astype(np.float32)   # (sorted: the first c are the valid ones)
    Ip = np.where(valid, np.take_along_axis(ids, order, axis=2), -1).astype(np.int64)
    return Dp, Ip


def _lexsort_reference(Dp, Ip, k):
    n_parts, nq, _ = Dp.shape
    allD = Dp.transpose(1, 0, 2).reshape(nq, -1)
    allI = Ip.transpose(1, 0, 2).reshape(nq, -1)
    D = np.full((nq, k), NEG_FILL, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        v = np.nonzero(allI[q] >= 0)[0]
        o = v[np.lexsort((allI[q, v], -allD[q, v]))[:k]]
        D[q, :o.size], I[q, :o.size] = allD[q, o], allI[q, o]
    return D, I


# (n_parts, nq, k) and the branch of launch_merge_lists each takes (kRankMergeKeys = 4096, kRankMergeParts = 64,
# kMaxMergeListKeys = 16384)
RANK_SHAPES = [(1, 9, 80),                     # single part = copy
               (2, 33, 80), (8, 257, 80),      # the production shape, more queries than one wave of workgroups
               (64, 300, 1),                   # k = 1, most parts
               (64, 5, 64), (8, 3, 512),       # exactly 4096 keys
               (51, 2, 80), (3, 7, 1365)]      # just below
SORT_SHAPES = [(3, 7, 1366),                   # 4098 keys: merge_lists<32> WITH status words
               (65, 4, 8),                     # more than 64 parts at 520 keys
               (8, 3, 2048),                   # 16384 keys: merge_lists<64>, 128 KiB of dynamic LDS
               (8, 2, 2049)]                   # radix path: status words through copy_status_words
# contents that must reach a rank-merge shape AND a sorting shape (check 2 needs both kernels on the same input)
SPECIAL_SHAPES = [(2, 33, 80), (8, 257, 80), (64, 5, 64), (3, 7, 1366), (65, 4, 8), (8, 2, 2049)]
SPECIALS = [("zeros", "short"), ("zeros", "full"), ("inf", "short"), ("inf", "full"), ("ties", "short_total"),
            ("ties", "all_empty"), ("ties", "disagree")]
MERGE_CASES = [(s, "ties", c) for s in RANK_SHAPES + SORT_SHAPES for c in ("full", "short")] + \
              [(s, sc, c) for s in SPECIAL_SHAPES for sc, c in SPECIALS]


@pytest.mark.parametrize("shape,scores,counts", MERGE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_gathered_merge_equals_lexsort_and_the_sorting_merge(gpu_device, shape, scores, counts):
    import torch
    from proqa_amd import _lib
    n_parts, nq, k = shape
    rng = np.random.default_rng(zlib.crc32(repr((shape, scores, counts)).encode()))
    Dp, Ip = _make_parts(rng, n_parts, nq, k, scores, counts)
    words = _status_words(n_parts)
    g = torch.from_numpy(_pack_blocks(Dp, Ip, words)).to(gpu_device)
    n_i, n_d, block = _layout(nq, k)
    status_host = _pinned_status(n_parts)
    D, I = _merge_gathered(g, n_parts, nq, k, status_host, gpu_device)
    torch.cuda.current_stream().synchronize()
    # 3. every part's status word, as its block held it
    assert _u32(status_host.tolist()) == words
    # 1. the NumPy reference; the rest of the row is I = -1, D = -FLT_MAX; no poison is left
    Dr, Ir = _lexsort_reference(Dp, Ip, k)
    np.testing.assert_array_equal(I.cpu().numpy(), Ir)
    np.testing.assert_array_equal(D.cpu().numpy(), Dr)          # by value: -0.0 == +0.0
    assert not (I == POISON_I).any() and not (D.view(torch.int32) == POISON_D).any()
    # 2. the sorting merge of the same buffer: same ids, same score BITS
    Ds, Is = _poisoned_out(nq, k, gpu_device)
    _lib.check(_lib.load().proqa_topk_merge_strided_device(g.data_ptr() + n_i, g.data_ptr(), n_parts, nq, k, block // 4, block // 8,
                                                           Ds.data_ptr(), Is.data_ptr(), _lib.current_stream_ptr()))
    assert torch.equal(I, Is) and torch.equal(D.view(torch.int32), Ds.view(torch.int32))
    # status_host = NULL is accepted and changes nothing
    Dn, In = _merge_gathered(g, n_parts, nq, k, None, gpu_device)
    assert torch.equal(I, In) and torch.equal(D.view(torch.int32), Dn.view(torch.int32))


def test_gathered_merge_without_queries_still_delivers_the_status_words(gpu_device):
    """nq = 0: nothing is merged, the blocks are a status word each"""
    import torch
    n_parts, nq, k = 8, 0, 80
    assert _layout(nq, k) == (0, 0, 16)
    words = _status_words(n_parts)
    g = torch.from_numpy(_pack_blocks(np.zeros((n_parts, 0, k), np.float32), np.zeros((n_parts, 0, k), np.int64), words)).to(gpu_device)
    status_host = _pinned_status(n_parts)
    D, I = _merge_gathered(g, n_parts, nq, k, status_host, gpu_device)
    torch.cuda.current_stream().synchronize()
    assert _u32(status_host.tolist()) == words
    assert (I == POISON_I).all() and (D.view(torch.int32) == POISON_D).all()      # no query: nothing written
    _merge_gathered(g, n_parts, nq, k, None, gpu_device)
    torch.cuda.current_stream().synchronize()


# ---- B. an N-rank sharded search in one process, real searches -----------------------------------------------------------

def _int_rows(rng, n):
    # integer-valued fp16: every partial sum is exact in fp32, ids and scores must match the oracle bit for bit
    return rng.integers(-4, 5, (n, 128)).astype(np.float16)


def _adversarial_rows(n, step=1.0):
    """the rows of test_rccl_gpu._adversarial: sorted by ascending score (with ties) for a query with q[0] = 1 -- every
    round's candidate lists overflow"""
    xb = np.zeros((n, 128), np.float16)
    xb[:, 0] = ((np.arange(n) // 40) * step).astype(np.float16)
    return xb


# Uneven shards of a 60 k-row corpus.  Leaping rounds need a bootstrap, i.e. a shard of >= 16384 rows, and on integer scores
# (ties in thousands) they fall short as a rule: CUTS_8 keeps every shard below that size, so that a status word of 1 is the
# test's doing; CUTS_LEAP has the one shard (the first) that leaps.
CUTS_8 = [0, 9000, 21000, 24003, 33000, 33700, 45011, 52555, 60000]
CUTS_LEAP = [0, 20000, 26000, 29003, 35000, 35700, 45011, 52555, 60000]


@functools.lru_cache(maxsize=None)
def _corpus(kind, nq):
    """(xb, xq, oracle D, oracle I) at k = 80; computed once, shared, never modified"""
    rng = np.random.default_rng(zlib.crc32(repr((kind, nq)).encode()))
    xb, xq = _int_rows(rng, 60000), _int_rows(rng, nq)
    if kind == "adversarial":            # shard 1 (12000 rows) in the adversarial order: scores 0 .. 299, the others reach ~300
        xb[CUTS_8[1]:CUTS_8[2]] = _adversarial_rows(CUTS_8[2] - CUTS_8[1])
        xq[:, 0] = 1
    else:
        assert kind == "plain"
    return (xb, xq) + search_oracle.topk_ip(xq, xb, 80)


def _handles(xb, bounds, device, nomination="auto", configure=None):
    import torch
    from proqa_amd.index import IndexFlatIP
    hs = []
    for p, (lo, hi) in enumerate(bounds):
        ix = IndexFlatIP(128)
        ix.configure_nomination(nomination)
        if configure and p in configure:
            ix.configure(*configure[p])
        if hi > lo:
            ix.add_device(torch.from_numpy(xb[lo:hi]).to(device))
        assert ix.ntotal == hi - lo
        ix.prepare()
        hs.append(ix)
    return hs


def _n_rank_search(hs, bounds, tq, k, device, warm=True):
    """The sequence of proqa_sharded_search_device over len(hs) ranks that share one receive buffer.  Returns (D, I, the status
    words after the first merge, the `rewritten` flags, the number of merges)."""
    import torch
    from proqa_amd import _lib
    lib = _lib.load()
    nq = tq.shape[0]
    if warm:   # the first search of a size allocates the workspace: _begin then really only enqueues
        for ix in hs:
            ix.search_device(tq, k)
    n_i, n_d, block = _layout(nq, k)
    gathered = torch.full((len(hs), block), 0xA5, dtype=torch.uint8, device=device)
    for p, (ix, (lo, _)) in enumerate(zip(hs, bounds)):
        base = gathered.data_ptr() + p * block
        _lib.check(lib.proqa_index_search_begin_device(ix._h, tq.data_ptr(), nq, 0, k, lo, base + n_i, base, base + n_i + n_d,
                                                       _lib.current_stream_ptr()))
    status_host = _pinned_status(len(hs))
    D, I = _merge_gathered(gathered, len(hs), nq, k, status_host, device)
    rewritten = []
    for ix in hs:
        r = ctypes.c_int(-1)
        _lib.check(lib.proqa_index_search_finish(ix._h, ctypes.byref(r)))
        rewritten.append(r.value)
    torch.cuda.current_stream().synchronize()
    first = _u32(status_host.tolist())
    merges = 1
    assert set(first) <= {0, 1}, first
    if 1 in first:   # some rank rewrote its list: zero the words, merge once more
        gathered[:, n_i + n_d:n_i + n_d + 4] = 0
        status_host.fill_(POISON_STATUS)
        D, I = _merge_gathered(gathered, len(hs), nq, k, status_host, device)
        torch.cuda.current_stream().synchronize()
        assert _u32(status_host.tolist()) == [0] * len(hs)
        merges = 2
    assert not (I == POISON_I).any() and not (D.view(torch.int32) == POISON_D).any()
    return D, I, first, rewritten, merges


def _unsharded(xb, tq, k, device):
    import torch
    from proqa_amd.index import IndexFlatIP
    ix = IndexFlatIP(128)
    ix.add_device(torch.from_numpy(xb).to(device))
    D, I = ix.search_device(tq, k)
    ix.close()
    return D, I


def _assert_exact(D, I, Du, Iu, Do, Io):
    """bit for bit the unsharded search AND the oracle"""
    import torch
    assert torch.equal(I, Iu) and torch.equal(D.view(torch.int32), Du.view(torch.int32))
    np.testing.assert_array_equal(I.cpu().numpy(), Io)
    np.testing.assert_array_equal(D.cpu().numpy().view(np.uint32), Do.view(np.uint32))


def _close(hs):
    for ix in hs:
        ix.close()


@pytest.mark.parametrize("nomination", ["auto", "off", "always"])
@pytest.mark.parametrize("nq", [70, 300])
def test_eight_uneven_shards_equal_the_unsharded_search(gpu_device, nq, nomination):
    """N = 8, both wave tiles; the int8 scan as configured (automatic mode leaves shards this small on the fp16 rows, "always"
    scans every shard's own int8 copy): shard-local copies, global ids, the rank merge at the production shape"""
    import torch
    xb, xq, Do, Io = _corpus("plain", nq)
    bounds = list(zip(CUTS_8[:-1], CUTS_8[1:]))
    tq = torch.from_numpy(xq).to(gpu_device)
    hs = _handles(xb, bounds, gpu_device, nomination)
    D, I, first, rewritten, merges = _n_rank_search(hs, bounds, tq, 80, gpu_device)
    assert (first, rewritten, merges) == ([0] * 8, [0] * 8, 1)
    if nomination == "always":
        assert all(ix.last_stats()["nomination"] for ix in hs)
    _assert_exact(D, I, *_unsharded(xb, tq, 80, gpu_device), Do, Io)
    _close(hs)


def test_short_one_row_and_empty_shards(gpu_device):
    """A shard with fewer than k rows, one with exactly 1 row and an EMPTY one (shard_bounds produces it whenever n_total <
    world_size): the empty handle's enqueued search reports a list of -1 with status 0."""
    import torch
    rng = np.random.default_rng(77)
    xb, xq = _int_rows(rng, 9000), _int_rows(rng, 33)
    bounds = [(0, 3000), (3000, 3037), (3037, 3038), (3038, 3038), (3038, 9000)]
    tq = torch.from_numpy(xq).to(gpu_device)
    hs = _handles(xb, bounds, gpu_device)
    D, I, first, rewritten, merges = _n_rank_search(hs, bounds, tq, 80, gpu_device)
    assert (first, rewritten, merges) == ([0] * 5, [0] * 5, 1)
    _assert_exact(D, I, *_unsharded(xb, tq, 80, gpu_device), *search_oracle.topk_ip(xq, xb, 80))
    # all shards short or empty: fewer rows than k in total
    few = [(0, 37), (37, 38), (38, 38), (38, 50)]
    hs2 = _handles(xb[:50], few, gpu_device)
    D, I, first, rewritten, merges = _n_rank_search(hs2, few, tq, 80, gpu_device)
    assert (first, rewritten, merges) == ([0] * 4, [0] * 4, 1)
    _assert_exact(D, I, *_unsharded(xb[:50], tq, 80, gpu_device), *search_oracle.topk_ip(xq, xb[:50], 80))
    assert (I[:, 50:] == -1).all() and (I[:, :50] >= 0).all()
    _close(hs + hs2)


def test_non_finite_scores_survive_the_rank_merge(gpu_device):
    """Rows with +inf, -inf and NaN spread over several shards (one shorter than k): the heap rule of the unsharded search"""
    import torch
    rng = np.random.default_rng(380)
    xb, xq = _int_rows(rng, 9000), _int_rows(rng, 70)
    xq[:, 0] = np.where(np.arange(70) % 2 == 0, 1.0, -1.0).astype(np.float16)      # sign decides +inf / -inf per query
    xq[:, 1] = 1.0
    for i, r in enumerate(rng.choice(9000, size=60, replace=False)):
        if i % 3 == 0:
            xb[r, 0] = np.inf
        elif i % 3 == 1:
            xb[r, 1] = np.nan
        else:
            xb[r, 0] = -np.inf
    xb[5, 0] = np.inf       # the short first shard holds one of each kind
    xb[6, 1] = np.nan
    xb[7, 0] = -np.inf
    bounds = [(0, 60), (60, 2500), (2500, 5000), (5000, 9000)]
    tq = torch.from_numpy(xq).to(gpu_device)
    hs = _handles(xb, bounds, gpu_device)
    D, I, first, rewritten, merges = _n_rank_search(hs, bounds, tq, 80, gpu_device)
    assert (first, rewritten, merges) == ([0] * 4, [0] * 4, 1)
    _assert_exact(D, I, *_unsharded(xb, tq, 80, gpu_device), *search_oracle.topk_ip_heap(xq, xb, 80))
    assert not torch.isnan(D).any() and torch.isposinf(D[:, 0]).all()
    _close(hs)


def test_an_overflowing_shard_asks_for_a_second_merge(gpu_device):
    """One shard in the adversarial order, with a round schedule that overflows: its status word is 1 after the first merge (the
    others' 0), its _finish rewrites its list (rewritten = 1 for it alone), the SECOND merge is the exact result."""
    import torch
    xb, xq, Do, Io = _corpus("adversarial", 70)
    bounds = list(zip(CUTS_8[:-1], CUTS_8[1:]))
    tq = torch.from_numpy(xq).to(gpu_device)
    hs = _handles(xb, bounds, gpu_device, configure={1: (128, 4)})
    D, I, first, rewritten, merges = _n_rank_search(hs, bounds, tq, 80, gpu_device)
    only_1 = [int(p == 1) for p in range(8)]
    assert (first, rewritten, merges) == (only_1, only_1, 2)
    assert [ix.last_stats()["fallback_rounds"] > 0 for ix in hs] == [bool(v) for v in only_1]
    _assert_exact(D, I, *_unsharded(xb, tq, 80, gpu_device), Do, Io)
    assert ((I >= CUTS_8[1]) & (I < CUTS_8[2])).any()           # the rewritten list matters to the result
    _close(hs)


def test_a_leap_that_falls_short_asks_for_a_second_merge(gpu_device, monkeypatch):
    """PROQA_LEAP_ROUNDS / PROQA_LEAP_RANK fixed as in test_leap_gpu.py: the one shard large enough for leaping rounds (shard
    0) tests against the score at rank 2, which fewer than k of its later rows beat -- its queries end the round short and are
    searched again in _finish.  Same status protocol."""
    import torch
    xb, xq, Do, Io = _corpus("plain", 70)
    bounds = list(zip(CUTS_LEAP[:-1], CUTS_LEAP[1:]))
    tq = torch.from_numpy(xq).to(gpu_device)
    Du, Iu = _unsharded(xb, tq, 80, gpu_device)
    hs = _handles(xb, bounds, gpu_device)
    hs[0].configure_leap("off")           # the workspace of this size, without a shortfall that would pause the leaps
    for ix in hs:
        ix.search_device(tq, 80)
    hs[0].configure_leap("auto")
    monkeypatch.setenv("PROQA_LEAP_RANK", "2")
    monkeypatch.setenv("PROQA_LEAP_ROUNDS", "1")
    D, I, first, rewritten, merges = _n_rank_search(hs, bounds, tq, 80, gpu_device, warm=False)
    only_0 = [int(p == 0) for p in range(8)]
    assert (first, rewritten, merges) == (only_0, only_0, 2)
    st = hs[0].last_stats()
    assert st["leap_rank"] == 2 and st["fallback_rounds"] > 0, st
    _assert_exact(D, I, Du, Iu, Do, Io)
    _close(hs)


def test_fifty_one_shards_stay_on_the_rank_merge(gpu_device):
    """N = 51 shards of a 6 k-row corpus at k = 80: 4080 keys per query"""
    import torch
    from proqa_amd.index import shard_bounds
    rng = np.random.default_rng(51)
    xb, xq = _int_rows(rng, 6000), _int_rows(rng, 33)
    bounds = [shard_bounds(6000, 51, r) for r in range(51)]
    tq = torch.from_numpy(xq).to(gpu_device)
    hs = _handles(xb, bounds, gpu_device)
    D, I, first, rewritten, merges = _n_rank_search(hs, bounds, tq, 80, gpu_device)
    assert (first, rewritten, merges) == ([0] * 51, [0] * 51, 1)
    _assert_exact(D, I, *_unsharded(xb, tq, 80, gpu_device), *search_oracle.topk_ip(xq, xb, 80))
    _close(hs)


# ---- C. ShardedIndexFlatIP._search_in_place with a world of 8 ------------------------------------------------------------

WORLD, C_ROWS, C_NQ, C_K = 8, 48000, 7, 3          # odd nq * k: the 16-byte padding of the block parts is exercised


class _StubDist:
    """What _search_in_place needs of torch.distributed.  The all-gather copies `mine` into row `rank` of the receive buffer
    and the peers' prepared blocks (script(call number) -> [WORLD, block] uint8 device tensor) into the other rows, with
    torch copies on the current stream: ordered like the real collective."""

    def __init__(self, rank, script):
        self.rank, self.script, self.calls = rank, script, 0

    def is_initialized(self):
        return True

    def get_backend(self, group=None):
        return "nccl"

    def all_gather_into_tensor(self, gathered, mine, group=None):
        blocks = self.script(self.calls)
        self.calls += 1
        assert gathered.shape == blocks.shape and mine.shape == blocks.shape[1:]
        for p in range(gathered.shape[0]):
            gathered[p].copy_(mine if p == self.rank else blocks[p])


def _world_rows(adversarial_rank=None):
    from proqa_amd.index import shard_bounds
    rng = np.random.default_rng(8 if adversarial_rank is None else 80 + adversarial_rank)
    xb, xq = _int_rows(rng, C_ROWS), _int_rows(rng, C_NQ)
    if adversarial_rank is not None:   # (scores 0, 2, .. 298: the shard's last rows are among the best of the corpus)
        lo, hi = shard_bounds(C_ROWS, WORLD, adversarial_rank)
        xb[lo:hi] = _adversarial_rows(hi - lo, step=2.0)
        xq[:, 0] = 1
    return xb, xq


def _peer_lists(xb, tq, device, rows=None):
    """every rank's own search_device(xq, k, idx_offset=lo) as numpy [WORLD, nq, k] arrays; rows: {rank: rows of its shard
    that it has searched so far}"""
    import torch
    from proqa_amd.index import IndexFlatIP, shard_bounds
    Dp, Ip = [], []
    for p in range(WORLD):
        lo, hi = shard_bounds(C_ROWS, WORLD, p)
        if rows and p in rows:
            hi = lo + rows[p]
        ix = IndexFlatIP(128)
        ix.add_device(torch.from_numpy(xb[lo:hi]).to(device))
        D, I = ix.search_device(tq, C_K, idx_offset=lo)
        Dp.append(D.cpu().numpy())
        Ip.append(I.cpu().numpy())
        ix.close()
    return np.stack(Dp), np.stack(Ip)


def _blocks(lists, words, device):
    import torch
    return torch.from_numpy(_pack_blocks(lists[0], lists[1], words)).to(device)


def _live_rank(xb, rank, dist, configure=None):
    """ShardedIndexFlatIP as rank `rank` of WORLD, constructed without a process group"""
    from proqa_amd.index import ShardedIndexFlatIP, shard_bounds
    index = ShardedIndexFlatIP(C_ROWS, preallocate=False)
    assert index.world_size == 1
    index.world_size, index.rank, index.dist = WORLD, rank, dist
    index.lo, index.hi = shard_bounds(C_ROWS, WORLD, rank)
    if configure:
        index.local_index.configure(*configure)
    index.add_local(xb[index.lo:index.hi])
    return index


def _assert_is(D, I, Du, Iu):
    import torch
    assert torch.equal(I, Iu) and torch.equal(D.view(torch.int32), Du.view(torch.int32))


@functools.lru_cache(maxsize=None)
def _world(device):
    """the healthy world: rows, queries, every rank's final list, the unsharded result"""
    import torch
    xb, xq = _world_rows()
    tq = torch.from_numpy(xq).to(device)
    return xb, tq, _peer_lists(xb, tq, device), _unsharded(xb, tq, C_K, device)


@pytest.mark.parametrize("rank", [0, 3, 7])
def test_in_place_search_with_final_peers_takes_one_collective(gpu_device, rank):
    xb, tq, final, (Du, Iu) = _world(gpu_device)
    healthy = _blocks(final, [0] * WORLD, gpu_device)
    dist = _StubDist(rank, lambda call: healthy)
    index = _live_rank(xb, rank, dist)
    D, I = index.search(tq, C_K)
    assert dist.calls == 1
    _assert_is(D, I, Du, Iu)
    index.close()


def test_in_place_search_repeats_the_exchange_for_its_own_overflow(gpu_device):
    import torch
    rank = 3
    xb, xq = _world_rows(adversarial_rank=rank)
    tq = torch.from_numpy(xq).to(gpu_device)
    healthy = _blocks(_peer_lists(xb, tq, gpu_device), [0] * WORLD, gpu_device)
    dist = _StubDist(rank, lambda call: healthy)
    index = _live_rank(xb, rank, dist, configure=(128, 4))
    D, I = index.search(tq, C_K)
    assert dist.calls == 2
    assert index.local_index.last_stats()["fallback_rounds"] > 0
    Du, Iu = _unsharded(xb, tq, C_K, gpu_device)
    _assert_is(D, I, Du, Iu)
    Do, Io = search_oracle.topk_ip(xq, xb, C_K)
    np.testing.assert_array_equal(I.cpu().numpy(), Io)
    np.testing.assert_array_equal(D.cpu().numpy(), Do)
    lo, hi = index.lo, index.hi
    assert ((I >= lo) & (I < hi)).any()            # the rewritten list matters to the result
    index.close()


def test_in_place_search_repeats_the_exchange_for_a_peer(gpu_device):
    """Peer 5 reports 1 with a sorted but incomplete list (its top-k over the first half of its rows) on the first call, then its
    final list with 0: two collectives, the exact result; a plain search on the same object afterwards is exact too."""
    import torch
    xb, tq, final, (Du, Iu) = _world(gpu_device)
    rank, peer = 2, 5
    half = _peer_lists(xb, tq, gpu_device, rows={peer: C_ROWS // WORLD // 2})
    assert not np.array_equal(half[1][peer], final[1][peer])
    early = _blocks(half, [int(p == peer) for p in range(WORLD)], gpu_device)
    healthy = _blocks(final, [0] * WORLD, gpu_device)
    dist = _StubDist(rank, lambda call: early if call == 0 else healthy)
    index = _live_rank(xb, rank, dist)
    D, I = index.search(tq, C_K)
    assert dist.calls == 2
    _assert_is(D, I, Du, Iu)
    D, I = index.search(tq, C_K)
    assert dist.calls == 3
    _assert_is(D, I, Du, Iu)
    index.close()


def test_in_place_search_names_a_poisoned_peer_and_recovers(gpu_device):
    xb, tq, final, (Du, Iu) = _world(gpu_device)
    rank, peer = 4, 6
    poisoned = _blocks(final, [K_POISON if p == peer else 0 for p in range(WORLD)], gpu_device)
    healthy = _blocks(final, [0] * WORLD, gpu_device)
    dist = _StubDist(rank, lambda call: poisoned if call == 0 else healthy)
    index = _live_rank(xb, rank, dist)
    with pytest.raises(RuntimeError, match=rf"rank {peer} failed"):
        index.search(tq, C_K)
    assert dist.calls == 1
    D, I = index.search(tq, C_K)
    assert dist.calls == 2
    _assert_is(D, I, Du, Iu)
    index.close()


def test_in_place_search_gives_up_when_a_peer_never_agrees(gpu_device):
    xb, tq, final, (Du, Iu) = _world(gpu_device)
    rank, peer = 0, 1
    stuck = _blocks(final, [int(p == peer) for p in range(WORLD)], gpu_device)
    healthy = _blocks(final, [0] * WORLD, gpu_device)
    dist = _StubDist(rank, lambda call: stuck if call < 2 else healthy)
    index = _live_rank(xb, rank, dist)
    with pytest.raises(RuntimeError, match="did not agree"):
        index.search(tq, C_K)
    assert dist.calls == 2
    D, I = index.search(tq, C_K)                   # the handle and its buffers stay usable
    assert dist.calls == 3
    _assert_is(D, I, Du, Iu)
    index.close()
