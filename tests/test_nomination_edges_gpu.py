"""The int8 nomination scan (mips_filter_i8, quantise_rows_i8, prep_queries_i8, lane_threshold / block_threshold) with rows AT
THE EDGE of its bound.  The corpora of nomination_corpora.py plant, per edge query, one row whose integer score lies below
the real per-block threshold A G_b - B - E X_b's own centre by a stated fraction of the rigorous margin B + E X_b
(nomination_oracle.py; test_nomination_oracle_host.py checks the constructions on the CPU and, with -s, prints this table):

    corpus       kind  gap / bound of the planted rows, rung by rung        what carries the margin
    b_edge       B     0.512  0.764  0.913  0.984  0.99994                  B = ||w / s_q|| R alone (e = 0); decoy rows
    e_edge       E     0.508  0.762  0.905  0.984  0.99998                  E X_b alone (R = 0), the row is its block's X_b
    both         BE    0.511  0.760  0.911  0.984  0.99999                  both terms, each at its Cauchy-Schwarz equality
    hetero       B     0.984  0.99994   blocks of 4 x smaller / larger f_b than both neighbours, 20011 rows: behind the
    hetero_e     E     0.984  0.99998   bootstrap, first / last units of chunks, the last full and the partial last block
    hetero_wide  E     0.984  0.99998   200011 rows: such blocks at units 3 | 4, 7 | 8 and last | 0 of 384- and 512-row chunks
    dim_scales   B     as b_edge, c_d = 16, 32, 64, 128 by dimension, q_d scaled inversely
    shifted      B     0.510  0.765  0.916  0.988                           |q.mean| = 4064 > 10 x the scores' spread
    const_zero   E     0.513  0.765  0.916  0.983  0.99998, seven constant dimensions; an all-zero query beside them

The kernel's documented inflation ((1 + 2^-10) factors, + 2^-6, 2^-20 A, delta) leaves the planted row nearest its
threshold 54 (hetero_e, hetero_wide) to 434 (dim_scales) integer units to spare, of a margin of 3400 .. 7060: a margin
narrower than ~98 % of the rigorous one loses rows here.  Every value lies on a power-of-two grid and every partial
sum fits 24 bits, so oracle/search_oracle.topk_ip_exact gives the only right bits and "equal" means equal, as in
test_filter_i8_stagger_gpu.py.  An edge query's k-th best score is its 128 anchors' T in every round, for every k <= 128.

Geometry (nomination_corpora.plan restates the library's rule -- growth_for, plan_slabs_equal, run_round's geometry; the
library exports no plan, so the tests assert what they can see of it: the device's 256 compute units and the number of
rounds).  At 20011 rows every chunk of every launch is ONE 128-row stage: one load of block constants, units 0..3.  The
staggered loop of a chunk is reached by hetero_wide alone: the last slab of a search of <= 256 queries is cut into chunks
of 384 rows (pair 0 = units 0..7 under one 64-byte load of block constants, pair 1 = units 8..11 under the next), that of
513 queries into chunks of 512 rows (two whole pairs; two query blocks per wave, block 1's test carried across the pair
barrier).  Its level-5 and level-1 blocks sit on both sides of the stage boundary inside pair 0, on both sides of the
pair boundary and at the chunk's two ends, for each of the two layouts.

`nominated` (mips_index.cpp: stats.nominated = the sum over queries of stat_nom, which topk_merge raises by the number of
nominee bits it collected for the query in a round, rows of the slab only) counts (query, row) pairs behind the
bootstrap whose integer score exceeded the block threshold of the round: with thresholds fixed at T it is bracketed by
the oracle's forced(T) and allowed(T).  On b_edge the two differ: decoy rows at 0.9 and 0.99 of the bound below T are
forced, those at 1.008 lie inside the kernel's inflation (either answer is right), those at 1.05 must stay out.  On the
other counted corpora forced = allowed = one pair per query: there the check says "the planted rows and nothing else".

Leaping rounds add little here and the header says so plainly: the planner leaps only at k = 128 (one round at rank 55), so
for k = 1 and 10 the "auto" searches repeat the "off" ones; and at k = 128 the tied anchors cannot pass a leaping round's own
verification ("the k-th best now beats the threshold it was handed"), so the edge queries fall short by the leap's rule
and are searched again on ordinary rounds (rescue_short_queries), which is the leap-less case once more.  fallback_rounds
then counts the rounds of that second search: the test works out from exact scores which queries fall short and demands
fallback_rounds == the rounds of a leap-less search of exactly those queries (0 where no leap is planned).

Replaces the same call site as every search test: retrieval/eval_retrieval.py:98-104 of the reference."""
import numpy as np
import pytest

import nomination_corpora as nc
import nomination_oracle as no
from oracle import search_oracle

pytestmark = pytest.mark.gpu

KS = (1, 10, 128)
_open = {}


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for ix in _open.values():
        ix.close()
    _open.clear()


def _index(name):
    if name not in _open:
        from proqa_amd.index import IndexFlatIP
        ix = IndexFlatIP(128)
        ix.configure_bootstrap(nc.BOOT)
        ix.add(nc.corpus(name).xb)
        _open[name] = ix
    return _open[name]


def _search(ix, tq, k, nomination, leap, idx_offset=0):
    ix.configure_nomination(nomination)
    ix.configure_leap(leap)                       # (also forgets any pause an earlier search earned)
    D, I = ix.search_device(tq, k, idx_offset=idx_offset)
    return D.cpu().numpy(), I.cpu().numpy(), ix.last_stats()


def _expected_fallback(ix, xq, S, k, st, leap):
    """0, or under an active leap the rounds of the second search of the queries whose k-th best does not beat the rank-j
    score of the bootstrap's rows (header)"""
    import torch
    if leap == "off" or not st["leap_rank"]:
        return 0
    kth = np.sort(S, axis=1)[:, -k]
    jth_boot = np.sort(S[:, :nc.BOOT], axis=1)[:, -st["leap_rank"]]
    short = np.flatnonzero(~(kth > jth_boot))
    if len(short) == 0:
        return 0
    _, _, st2 = _search(ix, torch.from_numpy(xq[short]).cuda(), k, "always", "off")
    assert st2["fallback_rounds"] == 0, st2
    return st2["rounds"]


def _three_ways(name, xq, pos, ks=KS, leaps=("off", "auto"), idx_offset=0, expect_overflow=False):
    """nomination "off" == "always" == topk_ip_exact, ids and score bits; every planted row in its query's result"""
    import torch
    cp, ix = nc.corpus(name), _index(name)
    tq = torch.from_numpy(xq).cuda()
    S = (xq.astype(np.float64) @ cp.xb.astype(np.float64).T).astype(np.float32)
    out = {}
    for k in ks:
        Do, Io = search_oracle.topk_ip_exact(xq.astype(np.float32), cp.xb.astype(np.float32), k)
        D0, I0, st0 = _search(ix, tq, k, "off", "off", idx_offset)
        assert not st0["nomination"], st0
        np.testing.assert_array_equal(I0, Io + idx_offset)
        np.testing.assert_array_equal(D0.view(np.int32), Do.view(np.int32))
        for leap in leaps:
            D1, I1, st1 = _search(ix, tq, k, "always", leap, idx_offset)
            print(f"{name} nq {len(xq)} k {k} leap {leap}: rounds {st1['rounds']} fallback {st1['fallback_rounds']} nominated "
                  f"{st1['nominated']} leap_rank {st1['leap_rank']}")
            assert st1["nomination"], st1
            np.testing.assert_array_equal(I1, Io + idx_offset)
            np.testing.assert_array_equal(D1.view(np.int32), Do.view(np.int32))
            for lane, i in pos.items():
                assert I1[lane, 0] == cp.planted[i] + idx_offset, (lane, i, I1[lane, :3])
            if expect_overflow:
                assert st1["fallback_rounds"] > 0, st1
            else:
                assert st1["fallback_rounds"] == _expected_fallback(ix, xq, S, k, st1, leap), st1
            out[(k, leap)] = st1
    return out


@pytest.mark.parametrize("nq", (1, 33, 128, 200, 300, 513))
@pytest.mark.parametrize("name", nc.NAMES)
def test_edge_rows_are_nominated_and_the_result_is_exact(gpu_device, name, nq):
    """k = 1, 10, 128 x leaps off / auto on batches of 1, 33, 128 (row-split launches with 1, 2, 4 query blocks), 200 (one block
    per wave), 300 (two blocks per wave) and 513 queries (two query tiles); edge queries in the first and last lanes of the
    32-query blocks, plain queries around them (nomination_corpora.EDGE_FILLED: edge queries in every lane).  Which edge
    queries a small batch holds rotates with the batch size."""
    cp = nc.corpus(name)
    xq, pos = nc.batch(cp, nq, rotate=(7 * nq) % len(cp.edge_q), fill="edge" if name in nc.EDGE_FILLED else "plain")
    _three_ways(name, xq, pos)


def test_an_index_offset_shifts_the_ids_and_nothing_else(gpu_device):
    cp = nc.corpus("hetero")
    xq, pos = nc.batch(cp, 300)
    _three_ways("hetero", xq, pos, ks=(10,), idx_offset=3_000_000_000)


def test_a_zero_query_beside_edge_queries(gpu_device):
    """The all-zero query nominates every row (A = 0: acc = 0 > -B), its merge overflows and the rounds are re-scanned by the
    overflow-safe path -- fallback_rounds > 0 by design (test_a_suspended_scan_is_probed_again_and_resumes); the edge
    queries of the same batch still get their planted rows and the oracle's bits."""
    cp = nc.corpus("const_zero")
    xq, pos = nc.batch(cp, 200, zero=True)
    assert not xq[1].any()
    _three_ways("const_zero", xq, pos, leaps=("off",), expect_overflow=True)


def test_edge_rows_in_the_second_of_two_shards(gpu_device):
    """Two indexes with their own quantiser each (an E corpus on other sign patterns in front), merged by merge_topk_device:
    the edge rows sit in the second shard, whose ids start at the first one's size."""
    import torch
    from proqa_amd.index import merge_topk_device
    first, cp = nc.corpus("front"), nc.corpus("b_edge")
    xq, pos = nc.batch(cp, 128)
    tq = torch.from_numpy(xq).cuda()
    n0 = len(first.xb)
    xb = np.concatenate([first.xb, cp.xb])
    for k in (1, 10, 128):
        Do, Io = search_oracle.topk_ip_exact(xq.astype(np.float32), xb.astype(np.float32), k)
        res = {}
        for mode in ("off", "always"):
            parts = []
            for name, off in (("front", 0), ("b_edge", n0)):
                ix = _index(name)
                ix.configure_nomination(mode)
                ix.configure_leap("off")
                parts.append(ix.search_device(tq, k, idx_offset=off))
                st = ix.last_stats()
                assert st["nomination"] == (mode == "always") and st["fallback_rounds"] == 0, st
            D, I = merge_topk_device(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
            res[mode] = (D.cpu().numpy(), I.cpu().numpy())
        for mode in res:
            np.testing.assert_array_equal(res[mode][1], Io)
            np.testing.assert_array_equal(res[mode][0].view(np.int32), Do.view(np.int32))
        for lane, i in pos.items():
            assert res["always"][1][lane, 0] == n0 + cp.planted[i]


def _count_check(name, nq, expect_rounds=None):
    import torch
    cp, ix = nc.corpus(name), _index(name)
    xq, pos = nc.batch(cp, nq, fill="edge")
    o = no.Oracle(cp.xb, cp.edge_q)
    forced = o.forced(cp.T)[:, nc.BOOT:].sum(axis=1)
    allowed = o.allowed(cp.T)[:, nc.BOOT:].sum(axis=1)
    which = np.array([pos[lane] for lane in range(nq)])
    lo, hi = int(forced[which].sum()), int(allowed[which].sum())
    D, I, st = _search(ix, torch.from_numpy(xq).cuda(), 10, "always", "off")
    print(f"{name} nq {nq}: forced {lo} <= nominated {st['nominated']} <= allowed {hi}; rounds {st['rounds']}")
    assert st["nomination"] and st["fallback_rounds"] == 0 and st["leap_rank"] == 0, st
    if expect_rounds is not None:
        assert st["rounds"] == expect_rounds, st
    np.testing.assert_array_equal(I[:, 0], cp.planted[which])
    assert lo <= st["nominated"] <= hi, (lo, st["nominated"], hi)
    assert hi <= 1.1 * lo + nq
    return lo, hi


def _mi355x_geometry():
    """the chunk layouts hetero_wide is built for are those of 256 compute units"""
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count == nc.CUS


@pytest.mark.parametrize("nq", (128, 200, 513))
def test_wide_chunks_edge_rows_at_stage_pair_and_chunk_boundaries(gpu_device, nq):
    """hetero_wide, k = 10, leaps off: 128 queries (row-split launch) and 200 (one query block per wave) scan 384-row chunks,
    513 (two blocks per wave, two query tiles) 512-row chunks.  Edge queries in the first and last lanes of the blocks, plain
    queries around them; nomination off == always for every query, == the float64 oracle for the first 64 lanes (the
    score matrix of all 513 would be 0.8 GB)."""
    import torch
    _mi355x_geometry()
    cp, ix = nc.corpus("hetero_wide"), _index("hetero_wide")
    xq, pos = nc.batch(cp, nq, rotate=(5 * nq) % len(cp.edge_q))
    tq = torch.from_numpy(xq).cuda()
    D0, I0, st0 = _search(ix, tq, 10, "off", "off")
    D1, I1, st1 = _search(ix, tq, 10, "always", "off")
    print(f"hetero_wide nq {nq}: rounds {st1['rounds']} fallback {st1['fallback_rounds']} nominated {st1['nominated']}")
    assert st1["nomination"] and not st0["nomination"] and st1["fallback_rounds"] == 0, st1
    assert st1["rounds"] == len(nc.plan(nc.N_WIDE, nq, 10)), st1
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1.view(np.int32), D0.view(np.int32))
    Do, Io = search_oracle.topk_ip_exact(xq[:64].astype(np.float32), cp.xb.astype(np.float32), 10)
    np.testing.assert_array_equal(I1[:64], Io)
    np.testing.assert_array_equal(D1[:64].view(np.int32), Do.view(np.int32))
    for lane, i in pos.items():
        assert I1[lane, 0] == cp.planted[i], (lane, i, cp.where[cp.planted[i] // 32], I1[lane, :3])


@pytest.mark.parametrize("nq", (24, 513))
def test_wide_chunks_nominated_count(gpu_device, nq):
    """hetero_wide's 24 edge queries once (a row-split launch over 384-row chunks) and tiled to 513 (512-row chunks, two query
    blocks per wave): nominated == one pair per query, no more.  A scan that took a unit's constants from the wrong place
    of its pair's load, or did not advance to the next pair's, loses the rows of the level-1 blocks (threshold 4 x too
    high) or nominates whole level-5 blocks' neighbours."""
    _mi355x_geometry()
    lo, hi = _count_check("hetero_wide", nq, expect_rounds=len(nc.plan(nc.N_WIDE, nq, 10)))
    assert lo == hi == nq


@pytest.mark.parametrize("tiled", (False, True), ids=("once", "tiled_to_300"))
@pytest.mark.parametrize("name", nc.COUNTED)
def test_the_nominated_count_lies_between_forced_and_allowed(gpu_device, name, tiled):
    """Leaps off, k = 10, batches of edge queries only (once each -- a row-split launch -- and 300 of them, two blocks per wave):
    every threshold is T in every round, so nominated must lie in [|forced(T)|, |allowed(T)|] over the rows behind the
    bootstrap.  A scan that reads another block's constants over-nominates (upper side) or loses planted rows; a
    shrunken margin falls below the lower side."""
    lo, hi = _count_check(name, 300 if tiled else len(nc.corpus(name).edge_q))
    assert (lo < hi) == (name == "b_edge")            # (the decoys inside the kernel's inflation)
