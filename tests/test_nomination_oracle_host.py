"""The int8 nomination bound on the CPU: nomination_oracle.py (the quantiser and its bound in float64) against the edge corpora of
nomination_corpora.py and against small samples of the distributions test_nomination_gpu.py searches.  No GPU: this pins the
ORACLE and the CONSTRUCTIONS that test_nomination_edges_gpu.py then holds the scan to.

The search these tests are about replaces retrieval/eval_retrieval.py:98-104 of the reference (`IndexFlatIP.search`).

Run with -s for the table of reached fractions (planted row by planted row: shortfall / bound, and gap / bound, the part of
the rigorous margin a scan must keep to nominate the row)."""
import numpy as np
import pytest

import nomination_corpora as nc
import nomination_oracle as no
from oracle import search_oracle

ALL = nc.NAMES + ("hetero_wide",)
_oracles = {}


def _oracle(name):
    """the corpus with ALL its queries: edge queries first, then the zero query (if any), then the plain ones"""
    if name not in _oracles:
        cp = nc.corpus(name)
        _oracles[name] = (cp, no.Oracle(cp.xb, np.concatenate([cp.edge_q, cp.extra_q, cp.plain_q])))
    return _oracles[name]


def _holds(o):
    sh, bd = o.shortfall(), o.row_bound()
    # (float64 rounding of the two sides: scores of ~1e7 integer units carry ~1e-8 of one)
    return float((np.abs(sh) - bd * (1 + 1e-12)).max()), sh, bd


@pytest.mark.parametrize("name", ALL)
def test_the_bound_holds_for_every_pair_of_an_edge_corpus(name):
    cp, o = _oracle(name)
    worst, sh, bd = _holds(o)
    assert worst <= 1e-6, worst
    # the identity behind it, term by term: shortfall = e.xi + (w / s_q).r
    q, r = o.queries, o.rows
    terms = q.e @ r.xi.T.astype(np.float64) + q.wn @ r.r.T
    assert np.abs(terms - sh).max() <= 1e-6 * max(1.0, float(np.abs(o.acc()).max()) * 1e-6)


@pytest.mark.parametrize("name", ALL)
def test_an_edge_corpus_is_what_its_header_says(name):
    cp, o = _oracle(name)
    r = o.rows
    # exact fp16 inputs are asserted where they are built; every partial sum of every dot product fits 24 bits
    ok, bits = no.partial_sums_fit_24_bits(np.concatenate([cp.edge_q, cp.extra_q, cp.plain_q]), cp.xb)
    assert ok, bits
    # the quantiser finds the designed grid: mean and c exact, block scales 128 * 2^level, background rows without residual
    assert (np.log2(r.c[r.c > 0]) % 1 == 0).all()
    np.testing.assert_array_equal(r.G[nc.SCALE_BLOCKS:], 128.0 * 2.0 ** cp.level[nc.SCALE_BLOCKS:])
    resid = np.sqrt((r.r ** 2).sum(axis=1))
    assert set(np.flatnonzero(resid > 0)) <= set(cp.planted), "only planted rows carry a residual"
    assert cp.xb.shape[0] % 32 != 0 and cp.xb.shape[0] >= 4 * nc.BOOT
    if name.startswith("hetero"):
        lv = cp.level
        for row in cp.planted:
            b = row // 32
            nb = [x for x in (b - 1, b + 1) if x < len(lv)]
            assert all(abs(lv[x] - lv[b]) >= 2 for x in nb), (row, lv[b], [lv[x] for x in nb])   # >= 4 x in f_b
            # (X_b: not between the partial last block and the last full one, which both hold a planted row)
            ratio = [r.X[x] / r.X[b] for x in nb if len(lv) - 1 not in (x, b)]
            assert all(v >= 2.5 for v in ratio) if lv[b] == 5 else all(v <= 1 / 2.5 for v in ratio), (row, ratio)
        if name == "hetero_wide":
            # every planted block sits at the unit of a chunk its layout says (plan(): the library's geometry rule)
            for b, (nq, u) in cp.where.items():
                r0, r1, rpc = nc.plan(nc.N_WIDE, nq, 10)[-1]
                assert r0 <= 32 * b < r1 and ((32 * b - r0) % rpc) // 32 == u and rpc == (384 if nq <= 256 else 512)
            assert sorted(cp.where) == sorted(set((cp.planted // 32).tolist()))
            assert {u for _, u in cp.where.values()} == {0, 3, 4, 7, 8, 11, 15}
        else:
            assert {cp.planted.max()} == {cp.xb.shape[0] - 1} and nc.BOOT in cp.planted
    if name in ("e_edge", "hetero_e", "hetero_wide", "const_zero"):
        xin = np.sqrt((r.xi.astype(np.float64) ** 2).sum(axis=1))
        np.testing.assert_array_equal(xin[cp.planted], r.X[cp.planted // 32])      # the largest-norm row of its block
    if name == "shifted":
        S = o.scores()[:len(cp.edge_q)]
        assert (np.abs(o.queries.off[:len(cp.edge_q)]) >= 10 * (S.max(axis=1) - S.min(axis=1)) / 2).all()
        assert (np.abs(o.queries.off[:len(cp.edge_q)]) >= 10 * np.abs(cp.T - o.queries.off[:len(cp.edge_q)])).all()
    if name == "dim_scales":
        assert len(set(r.c.tolist())) == 4
    if name == "const_zero":
        assert (r.c == 0).sum() == 7 and (r.xi[:, r.c == 0] == 0).all() and not cp.extra_q.any()


@pytest.mark.parametrize("name", ALL)
def test_every_planted_row_sits_at_its_rung(name):
    cp, o = _oracle(name)
    ne = len(cp.edge_q)
    S = o.scores()[:ne]
    sh, bd, acc, units = o.shortfall()[:ne], o.row_bound()[:ne], o.acc()[:ne], o.units()[:ne]
    print(f"\n{name}: R = {o.rows.R:.4f}")
    print("  query kind rung  level   row  pos  shortfall/bound  gap/bound  eps[int units]  bound[int units]")
    for i in range(ne):
        row = cp.planted[i]
        gap = (cp.T[i] - o.queries.off[i]) * units[i, row] - acc[i, row]
        print(f"  {i:5d} {cp.kinds[i]:>4s} {cp.declared[i]:5.3f} {cp.level[row // 32]:5d} {row:6d} {row % 32:3d}  {sh[i, row] / bd[i, row]:14.5f} "
              f"{gap / bd[i, row]:10.5f} {(cp.planted_score[i] - cp.T[i]) * units[i, row]:14.4f} {bd[i, row]:16.1f}")
        # the declared fraction of the bound, as shortfall and as the gap to the real threshold
        assert sh[i, row] >= cp.declared[i] * bd[i, row] and gap >= cp.declared[i] * bd[i, row]
        # T + eps with eps below one integer unit; 128 anchors at T inside the bootstrap; nothing else reaches T
        assert cp.T[i] < cp.planted_score[i] == S[i, row] and (cp.planted_score[i] - cp.T[i]) * units[i, row] <= 1.0
        assert (S[i, :nc.BOOT] == cp.T[i]).sum() == nc.ANCHORS and (S[i, :nc.BOOT] > cp.T[i]).sum() == 0
        assert (S[i, nc.BOOT:] >= cp.T[i]).sum() == 1
        assert np.float32(cp.T[i]) == cp.T[i] and np.float32(S[i, row]) == S[i, row]
    for k in (1, 10, 128):
        D, I = search_oracle.topk_ip_exact(cp.edge_q.astype(np.float32), cp.xb.astype(np.float32), k)
        np.testing.assert_array_equal(I[:, 0], cp.planted)


@pytest.mark.parametrize("name", nc.COUNTED)
def test_the_two_sides_of_the_count_check_are_tight(name):
    cp, o = _oracle(name)
    ne = len(cp.edge_q)
    tau = np.concatenate([cp.T, np.zeros(len(o.queries.off) - ne)])
    forced, allowed = o.forced(tau)[:ne, nc.BOOT:], o.allowed(tau)[:ne, nc.BOOT:]
    assert not (forced & ~allowed).any()
    assert allowed.sum() <= 1.1 * forced.sum() + ne, (forced.sum(), allowed.sum())
    assert forced[np.arange(ne), cp.planted - nc.BOOT].all()
    print(f"\n{name}: forced {forced.sum()} allowed {allowed.sum()} pairs of {ne} queries x {forced.shape[1]} rows")


def test_the_plan_mirror_gives_one_stage_chunks_at_20011_rows_and_three_or_four_stages_at_200011():
    for nq in (1, 33, 128, 200, 300, 513):
        for k in (1, 10, 128):
            assert all(rpc == 128 and r0 % 128 == 0 for r0, r1, rpc in nc.plan(nc.N_ROWS, nq, k))
    assert [len(nc.plan(nc.N_ROWS, nq, 10)) for nq in (1, 200, 300, 513)] == [1, 1, 2, 2]
    assert nc.plan(nc.N_WIDE, 128, 10) == [(4096, 28672, 128), (28672, 200011, 384)]
    assert nc.plan(nc.N_WIDE, 24, 10) == nc.plan(nc.N_WIDE, 200, 10) == nc.plan(nc.N_WIDE, 128, 10)
    assert nc.plan(nc.N_WIDE, 513, 10)[-1] == (75776, 200011, 512) and len(nc.plan(nc.N_WIDE, 513, 10)) == 4


def test_the_decoys_of_the_b_edge_corpus_lie_on_both_sides_of_the_bound():
    cp, o = _oracle("b_edge")
    forced, allowed = o.forced(np.concatenate([cp.T, np.zeros(len(o.queries.off) - len(cp.T))])), None
    allowed = o.allowed(np.concatenate([cp.T, np.zeros(len(o.queries.off) - len(cp.T))]))
    got = [(bool(forced[i, r]), bool(allowed[i, r])) for i, r in enumerate(cp.decoy_rows)]
    assert got == [(True, True)] * 4 + [(False, True)] * 2 + [(False, False)] * 2      # 0.9, 0.99 | 1.008 | 1.05 of the bound
    assert (o.scores()[np.arange(len(got)), cp.decoy_rows] < cp.T[:len(got)]).all()


def test_edge_rows_rotate_through_all_32_positions_of_their_blocks():
    assert {int(r) % 32 for name in nc.NAMES for r in nc.corpus(name).planted} == set(range(32))


def test_batches_put_edge_queries_into_first_and_last_lanes():
    cp = nc.corpus("b_edge")
    for nq in (1, 33, 128, 200, 300, 513):
        xq, pos = nc.batch(cp, nq, rotate=3)
        assert xq.shape == (nq, 128) and 0 in pos
        for lane, i in pos.items():
            assert lane % 32 in (0, 31) or lane == nq - 1
            np.testing.assert_array_equal(xq[lane], cp.edge_q[i])
        if nq >= 64:
            assert {0, 31, 32, 63} <= set(pos)
    xq, pos = nc.batch(cp, 300, fill="edge")
    assert len(pos) == 300 and (xq[len(cp.edge_q)] == cp.edge_q[0]).all()


@pytest.mark.parametrize("dist", ["normal", "shifted", "anisotropic", "constant_dims", "tiny", "huge"])
def test_the_bound_holds_on_samples_of_the_float_corpora(dist):
    """the six distributions of test_float_corpora_bit_identical_to_the_fp16_scan, 3001 rows (a partial last block of 25) x 64
    queries"""
    rng = np.random.default_rng(5)
    n, nq = 3001, 64
    xb = rng.standard_normal((n, 128)).astype(np.float32)
    xq = rng.standard_normal((nq, 128)).astype(np.float32)
    if dist == "shifted":
        xb += 20.0
    elif dist == "anisotropic":
        xb *= np.exp(rng.uniform(-4, 4, 128)).astype(np.float32)
    elif dist == "constant_dims":
        xb[:, ::3] = 7.5
        xb[:, 1] = 2000.0
    elif dist == "tiny":
        xb *= 1e-3
        xq *= 1e-2
    elif dist == "huge":
        xb *= 40.0
        xq *= 8.0
    o = no.Oracle(xb.astype(np.float16), xq.astype(np.float16))
    sh, bd = o.shortfall(), o.row_bound()
    # float64 rounding of (q.x - q.mean) G / s_q: relative 2^-52 of |q.x| + |q.mean| in integer units
    tol = 2.0 ** -44 * (np.abs(o.scores()) + np.abs(o.queries.off)[:, None]) * o.units() + 1e-9
    assert (np.abs(sh) <= bd + tol).all(), float((np.abs(sh) - bd).max())
    assert float((np.abs(sh) / np.maximum(bd, 1e-300)).max()) > 0.02     # (not vacuous: the bound is within two orders)
    # forced is a subset of allowed at any threshold, e.g. each query's 10th best score
    tau = np.sort(o.scores(), axis=1)[:, -10]
    assert not (o.forced(tau) & ~o.allowed(tau)).any()
    # and no row that beats the threshold lies below the real one: the scan can miss none
    assert not ((o.scores() > tau[:, None]) & ~o.forced(tau)).any()
