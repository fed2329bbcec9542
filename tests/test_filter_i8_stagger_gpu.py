"""The staggered unit loop of the two-block int8 nomination scan (mips_filter_i8<2>: the test of one query block runs under
the other block's MFMA chain, block 1's half a unit late -- across the pair barrier, and behind the loop for the chunk's last
unit) must stay invisible: ids and score bits are those of the same index under configure_nomination("off") AND those of
oracle/search_oracle.topk_ip_exact, exactly, in every case.

Replaces the same call site as every search test: retrieval/eval_retrieval.py:98-104 of the reference.

Inputs: N(0,1) rows and queries clipped to +-6 and rounded to the grid of 1/32 (exact in fp16).  Every product is then a
multiple of 2^-10 and every partial sum of a 128-long dot product stays below 2^13 (random rows: <= 128 * 36; planted rows:
2 |q|^2 ~ 256), i.e. within 24 bits: the fp32 sums of the scan are exact whatever their order, so the float64 oracle's
bits are the only right answer and "equal" can mean equal.  A planted winner of query q is the row 2 q (score ~256 against
~55 for the best random row).

Shapes: 69001 rows (>= 65536, so the default mode takes the int8 rounds; not a multiple of 32) x 320 queries (one 512-query
tile: two query blocks per wave, waves 5..7 padding only), k = 80 and k = 1; the planted queries are those of wave 1
(queries 64..95 = its block 0, 96..127 = its block 1).  The dense bootstrap is pinned to the first 4096 rows, the planted
rows start at 12288: inside the rounds' slabs.  A slab of <= 69001 rows is cut into chunks of <= 384 rows (12 units), so a
run of 640 consecutive rows covers every unit of two pairs, both sides of pair boundaries and the first units of chunks.

The lane-list cap (32 records per query, accumulator half and chunk) cannot be reached on chunks of 12 units: that case
alone uses 600000 rows and 513 queries (two query tiles: half as many chunks per slab, more than 32 units each in the last
slab), and checks the oracle for the planted query and the 31 queries after it (the float64 score matrix of all 513 would
be 2.5 GB)."""
import numpy as np
import pytest

from oracle import search_oracle

pytestmark = pytest.mark.gpu

N_ROWS = 69001
N_QUERIES = 320
BOOT = 4096
R0 = 3 * BOOT
WAVE_Q0 = 64          # first query of wave 1

_cache = {}


def _grid(rng, shape):
    return (np.rint(np.clip(rng.standard_normal(shape), -6, 6) * 32) / 32).astype(np.float16)


def _data():
    if "data" not in _cache:
        rng = np.random.default_rng(2300)
        _cache["data"] = (_grid(rng, (N_ROWS, 128)), _grid(rng, (511, 128)))
    return _cache["data"]


def _planted(xq, q):
    return (xq[q].astype(np.float32) * 2).astype(np.float16)


def _search_three_ways(xb, xq, k, expect_fallback=False, oracle_queries=None):
    """int8 rounds == fp16 scan == oracle, ids and score bits; returns the int8 search's (D, I, stats)"""
    import torch
    from proqa_amd.index import IndexFlatIP
    ix = IndexFlatIP(128)
    ix.configure_bootstrap(BOOT)
    ix.add(xb)
    tq = torch.from_numpy(xq).cuda()
    D1, I1 = ix.search_device(tq, k)
    st1 = ix.last_stats()
    D1, I1 = D1.cpu().numpy(), I1.cpu().numpy()
    ix.configure_nomination("off")
    D0, I0 = ix.search_device(tq, k)
    st0 = ix.last_stats()
    D0, I0 = D0.cpu().numpy(), I0.cpu().numpy()
    ix.close()
    print(f"rows {len(xb)} queries {len(xq)} k {k}: int8 rounds {st1['rounds']} fallback {st1['fallback_rounds']} nominated {st1['nominated']}")
    assert st1["nomination"] and not st0["nomination"], (st1, st0)
    if expect_fallback:
        assert st1["fallback_rounds"] > 0, st1
    else:
        assert st1["fallback_rounds"] == 0, st1
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1.view(np.int32), D0.view(np.int32))
    qs = np.arange(len(xq)) if oracle_queries is None else np.asarray(oracle_queries)
    Do, Io = search_oracle.topk_ip_exact(xq[qs].astype(np.float32), xb.astype(np.float32), k)
    np.testing.assert_array_equal(I1[qs], Io)
    np.testing.assert_array_equal(D1[qs].view(np.int32), Do.view(np.int32))
    return D1, I1, st1


@pytest.mark.parametrize("k", (80, 1))
def test_planted_winners_on_a_sliding_row_offset(gpu_device, k):
    """Query 64 + j's winner at row R0 + 64 s + (5 j + 3 s) % 64, s = 0..9: the 640 rows from R0 on are each the winner of some
    lane of wave 1 once, in both query blocks, with the lane <-> row-of-the-unit pairing changing from search to search."""
    xb0, xq_all = _data()
    xq = xq_all[:N_QUERIES]
    for s in range(10):
        xb = xb0.copy()
        rows = R0 + 64 * s + (5 * np.arange(64) + 3 * s) % 64
        assert len(set(rows.tolist())) == 64
        for j, r in enumerate(rows):
            xb[r] = _planted(xq, WAVE_Q0 + j)
        # (the oracle for wave 1 and the two waves around it; all 320 queries are compared with the fp16 scan)
        D, I, _ = _search_three_ways(xb, xq, k, oracle_queries=np.arange(0, 192))
        np.testing.assert_array_equal(I[WAVE_Q0:WAVE_Q0 + 64, 0], rows)


@pytest.mark.parametrize("k", (80, 1))
def test_planted_winners_in_the_last_rows_of_the_index(gpu_device, k):
    """The last 40 rows of 69001 (the chunk's last units, the last one partial: 69001 = 2156 * 32 + 9): block 1's test behind
    the loop, the tail clip with the deferred unit's row number, a one-stage last pair.  Row n - 40 + i is the winner of
    query 64 + 32 (i % 2) + i // 2: the two blocks alternate row by row."""
    xb0, xq_all = _data()
    xq = xq_all[:N_QUERIES]
    xb = xb0.copy()
    qs = np.array([WAVE_Q0 + 32 * (i % 2) + i // 2 for i in range(40)])
    rows = N_ROWS - 40 + np.arange(40)
    for q, r in zip(qs, rows):
        xb[r] = _planted(xq, q)
    D, I, _ = _search_three_ways(xb, xq, k)
    np.testing.assert_array_equal(I[qs, 0], rows)


@pytest.mark.parametrize("k", (80, 1))
def test_lane_twins_in_the_same_and_in_adjacent_units(gpu_device, k):
    """Query 64 + l (block 0) and its lane twin 96 + l (block 1): l = 0..7 win in the SAME 32-row unit (both branches taken back
    to back), l = 8..15 block 0 in one unit and block 1 in the next, l = 16..23 block 1 first and block 0 in the next unit."""
    xb0, xq_all = _data()
    xq = xq_all[:N_QUERIES]
    xb = xb0.copy()
    want = {}
    for l in range(24):
        u = R0 + 1024 + 96 * l          # a 32-aligned row, three units per twin pair (offsets from chunk starts vary with l)
        if l < 8:
            want[WAVE_Q0 + l], want[WAVE_Q0 + 32 + l] = u + 3 + l, u + 20 + l % 4
        elif l < 16:
            want[WAVE_Q0 + l], want[WAVE_Q0 + 32 + l] = u + l, u + 32 + l
        else:
            want[WAVE_Q0 + 32 + l], want[WAVE_Q0 + l] = u + l, u + 32 + l
    assert len(set(want.values())) == len(want)
    for q, r in want.items():
        xb[r] = _planted(xq, q)
    D, I, _ = _search_three_ways(xb, xq, k)
    for q, r in want.items():
        assert I[q, 0] == r, (q, r, I[q, :3])


@pytest.mark.parametrize("nq", (257, 511))
def test_batches_with_padding_lanes_beside_live_lanes(gpu_device, nq):
    """257 queries: wave 4 holds ONE live lane (threshold finite) beside 63 padding lanes (+inf); 511: one padding lane in the
    tile's last wave.  Planted winners for the last live queries, in adjacent rows."""
    xb0, xq_all = _data()
    xq = xq_all[:nq]
    xb = xb0.copy()
    qs = np.arange(nq - 3, nq)
    rows = R0 + 4992 + 31 + np.arange(3)      # the last row of one unit and the first two of the next
    for q, r in zip(qs, rows):
        xb[r] = _planted(xq, q)
    D, I, _ = _search_three_ways(xb, xq, 80)
    np.testing.assert_array_equal(I[qs, 0], rows)


def test_a_lane_list_driven_to_its_cap(gpu_device):
    """80 near-duplicates of query 70's winner, one per 32-row unit over 80 consecutive units of the last slab of 600000 rows
    (513 queries are two query tiles: 256 chunks per slab, so the last slab's chunks hold more than 32 units and at least 40 of
    the run's units fall into one chunk: more than 32 records for one lane list).  The overflow flag rises, the round is
    re-scanned by the fp16 path, and the result is still exact."""
    rng = np.random.default_rng(2301)
    n, nq, k = 600000, 513, 80
    xb = _grid(rng, (n, 128))
    xq = _grid(rng, (nq, 128))
    base = _planted(xq, 70).astype(np.float32)
    rows = n - 4096 + 32 * np.arange(80) + 1          # row 1 of each unit: the same accumulator half every time
    for i, r in enumerate(rows):
        dup = base.copy()
        dup[i] -= 1.0 / 32                            # near-duplicates with distinct scores
        xb[r] = dup.astype(np.float16)
    D, I, st = _search_three_ways(xb, xq, k, expect_fallback=True, oracle_queries=np.arange(70, 102))
    assert set(I[70].tolist()) == set(rows.tolist())
