"""IndexIVFFlat without a GPU: the NumPy IVF oracle against brute-force definitions, and the refusals that come before
any GPU work (k, nprobe, the quantizer, the command line).  Below those: the worlds of tests/test_ivf_edges_gpu.py are
exact in fp32 and have the shapes they claim, the table behind GAMMA is recomputed, and a NumPy model of the scan's and
the merge's list protocol shows which defect each world catches."""
import numpy as np
import pytest

import ivf_oracle


def _corpus(rng, n, nlist):
    x = rng.integers(-4, 5, (n, 128)).astype(np.float32)
    cent = rng.integers(-3, 4, (nlist, 128)).astype(np.float32)
    return x, cent


def test_oracle_probing_every_list_is_the_exact_l2_top_k():
    rng = np.random.default_rng(0)
    x, cent = _corpus(rng, 400, 6)
    xq = rng.integers(-4, 5, (9, 128)).astype(np.float32)
    a = ivf_oracle.assign(x, cent)
    for nprobe in (6, 11):
        D, I = ivf_oracle.search(xq, x, a, cent, nprobe, 17)
        Db, Ib = ivf_oracle.brute_l2(xq, x, 17)
        np.testing.assert_array_equal(I, Ib)
        np.testing.assert_array_equal(D, Db)


def test_oracle_one_probe_returns_rows_of_the_best_list_only():
    rng = np.random.default_rng(1)
    x, cent = _corpus(rng, 500, 5)
    xq = rng.integers(-4, 5, (12, 128)).astype(np.float32)
    a = ivf_oracle.assign(x, cent)
    D, I = ivf_oracle.search(xq, x, a, cent, 1, 8)
    best = np.argmax(xq.astype(np.float64) @ cent.astype(np.float64).T, axis=1)
    for q in range(len(xq)):
        live = I[q] >= 0
        assert (a[I[q][live]] == best[q]).all()
        assert (np.diff(D[q][live]) >= 0).all()


def test_oracle_fills_a_short_result():
    rng = np.random.default_rng(2)
    x, cent = _corpus(rng, 30, 4)
    xq = rng.integers(-4, 5, (5, 128)).astype(np.float32)
    a = ivf_oracle.assign(x, cent)
    D, I = ivf_oracle.search(xq, x, a, cent, 1, 64)
    probes = ivf_oracle.coarse(xq, cent, 1)[:, 0]
    for q in range(len(xq)):
        m = int((a == probes[q]).sum())
        assert (I[q, :m] >= 0).all() and (I[q, m:] == -1).all()
        assert (D[q, m:] == ivf_oracle.FLT_MAX).all()


def test_oracle_coarse_ties_go_to_the_lowest_list():
    cent = np.zeros((4, 128), np.float32)
    cent[1, 0] = cent[3, 0] = 1.0
    xq = np.zeros((1, 128), np.float32)
    xq[0, 0] = 2.0
    np.testing.assert_array_equal(ivf_oracle.coarse(xq, cent, 3), [[1, 3, 0]])


def test_search_flags_parse():
    from proqa_amd.predict_qa import build_parser
    p = build_parser()
    a = p.parse_args(["--do_predict"])
    assert (a.search, a.nlist, a.nprobe) == ("exact", 100, 20)
    a = p.parse_args(["--do_predict", "--search", "ivf", "--nlist", "64", "--nprobe", "7"])
    assert (a.search, a.nlist, a.nprobe) == ("ivf", 64, 7)
    with pytest.raises(SystemExit):
        p.parse_args(["--do_predict", "--search", "hnsw"])


@pytest.mark.parametrize("argv", [["--eval-k", "129"], ["--eval-k", "0"], ["--nprobe", "0"], ["--nlist", "0"]])
def test_cli_refuses_ivf_settings_before_gpu_work(argv):
    from proqa_amd.predict_qa import build_parser, check_search_args
    args = build_parser().parse_args(["--do_predict", "--search", "ivf"] + argv)
    with pytest.raises(SystemExit):
        check_search_args(args)
    check_search_args(build_parser().parse_args(["--do_predict", "--eval-k", "5000"]))   # exact: any k


@pytest.mark.parametrize("quantizer", [None, object(), "IndexFlatIP"])
def test_non_flat_quantizer_is_refused(quantizer):
    from proqa_amd.index import IndexIVFFlat
    with pytest.raises(TypeError):
        IndexIVFFlat(quantizer, 128, 10)


@pytest.mark.parametrize("k,nprobe", [(129, 1), (0, 1), (5, 0), (5, -3)])
def test_search_arguments_are_refused_before_gpu_work(k, nprobe):
    from proqa_amd.index import IndexIVFFlat
    index = object.__new__(IndexIVFFlat)    # no handle, no GPU: the checks come first
    index.d, index.nprobe = 128, nprobe
    with pytest.raises(ValueError, match="k=|nprobe="):
        index.search(np.zeros((2, 128), np.float32), k)


# ---------------------------------------------------------------------------------------------------------------------
# the worlds of tests/test_ivf_edges_gpu.py: what they are, and what they catch
# ---------------------------------------------------------------------------------------------------------------------
WORLDS = ivf_oracle.integer_worlds()


@pytest.fixture(scope="module")
def built():
    """every integer world, built once: name -> (x, cent, xq, assignment)"""
    out = {}
    for name, (make, _, _) in WORLDS.items():
        x, cent, xq = make()
        out[name] = (x, cent, xq, ivf_oracle.assign(x, cent))
    return out


def _scores(x, xq):
    x64, q64 = x.astype(np.float64), xq.astype(np.float64)
    return q64 @ x64.T - (x64 ** 2).sum(1)[None] / 2


def test_every_integer_world_is_exact_in_fp32(built):
    for name, (x, cent, xq, _) in built.items():
        assert ivf_oracle.exact_in_fp32(xq, x, cent), name
    x, cent, xq = ivf_oracle.nonfinite_world()
    assert ivf_oracle.exact_in_fp32(xq, x, cent)
    assert np.isfinite(x.astype(np.float32)).all(1).sum() == 220


def test_line_worlds_have_the_order_they_claim(built):
    for name, (x, _, xq, a) in built.items():
        if not name.startswith(("line-", "chunks-")) or "plateau" in name:
            continue
        assert (a == 0).all(), name
        step = np.diff(_scores(x, xq), axis=1)
        order = name.split("-")[1]
        if order == "ascending":
            assert (step > 0).all(), name                          # every row beats all rows before it, for every query
        elif order == "descending":
            assert (step < 0).all(), name
        elif order == "identical":
            assert (step == 0).all() and (x == x[0]).all(), name
        elif order == "mixed":
            assert (step[0::2] > 0).all() and (step[1::2] < 0).all(), name
    x, _, xq, _ = built["chunks-edges"]
    best = np.argmax(_scores(x, xq), axis=1)
    assert set(best) == set(ivf_oracle.CHUNK_EDGE_ROWS)            # each chunk-edge row is some query's nearest row
    top5 = np.argsort(-_scores(x, xq), axis=1)[:, :5]
    assert all(set(r) == set(ivf_oracle.CHUNK_EDGE_ROWS) for r in top5)


def test_ascending_rows_fill_a_list_to_exactly_256_at_k_128(built):
    """the capacity edge: at k = 128 every step of an ascending list loses its 128 keys, and all of them come back"""
    for name in ("line-ascending-385", "line-ascending-4097", "chunks-ascending"):
        x, cent, xq, a = built[name]
        trace = {}
        ivf_oracle.model_search(xq, x, a, cent, 1, 128, trace=trace)
        assert trace["longest_after_reappend"] == 256 and trace["cuts"] >= 1, (name, trace)
    for name in ("line-random-4097", "line-descending-4097"):      # ... which other orders do not reach
        x, cent, xq, a = built[name]
        trace = {}
        ivf_oracle.model_search(xq, x, a, cent, 1, 128, trace=trace)
        assert trace["longest_after_reappend"] < 256, (name, trace)


def test_merge_and_coarse_worlds_reach_their_edges(built):
    for name in ("merge-last", "merge-first"):
        x, cent, xq, a = built[name]
        sizes = np.bincount(a, minlength=64)
        assert sizes.min() >= 130 and sizes.max() <= 170
        probes = ivf_oracle.coarse(xq, cent, 64)
        assert (probes[:20] == np.arange(64)).all() and (probes[20:] != np.arange(64)).any()
        _, I = ivf_oracle.search(xq[:20], x, a, cent, 64, 128)
        where = a[I]                                                # the lists of the winners
        assert (where >= 56).all() if name == "merge-last" else (where <= 7).all()
        assert 64 > (4096 - 128) // 128 * 2 and 64 > (4096 - 80) // 80       # three batches at k = 128, two at k = 80
    x, cent, xq, a = built["sign"]
    sizes = np.bincount(a, minlength=4096)
    assert (sizes > 0).sum() == 3840 and (sizes[7::16] == 0).all()
    probes = ivf_oracle.coarse(xq, cent, 1024)
    assert (sizes[probes[0]] > 0).all() and (sizes[probes[1:]] == 0).any()
    for nlist in (100, 257):
        cent = built[f"coarse-{nlist}"][1]
        assert (cent[5] == cent[2]).all() and (cent[40] == cent[17]).all() and (cent[7] == 0).all()
        a = built[f"coarse-{nlist}"][3]
        assert (a != 5).all() and (a != 40).all() and (a == 2).any() and (a == 17).any()   # the lower list gets the rows
    x, cent, xq, _ = built["coarse-257"]
    assert ((xq.astype(np.float64) @ cent.astype(np.float64).T).max(1) <= 0).sum() >= 13


def test_kstep_ratio_table_and_gamma():
    for name in ivf_oracle.FLOAT_WORLDS:
        x, _, xq = ivf_oracle.float_world(name)
        assert xq.shape == (192, 128) and x.shape == (2000, 128)
        got = ivf_oracle.kstep_ratio(xq, x)
        print(f"{name}: worst |a32 - q.x| / (u sum|q x|) = {got:.4f}")
        assert round(got, 3) == ivf_oracle.KSTEP_RATIO[name]
    assert ivf_oracle.GAMMA == 4 * 2.770
    x, _, xq = ivf_oracle.float_world("normal")
    exact = ((x.astype(np.float64) - xq[70].astype(np.float64)) ** 2).sum(1)
    assert (ivf_oracle.distance_bound(xq[70], x) < 1e-3 * np.maximum(exact, 1)).all()     # a bound, not a tolerance


def _searches(name):
    _, nprobes, ks = WORLDS[name]
    if ks == ivf_oracle.LINE_KS:
        ks = (1, 80, 128)                   # (the model is slow: half of the GPU test's k values)
    return [(nprobe, k) for nprobe in nprobes for k in ks]


def test_models_without_a_defect_equal_the_oracle_on_every_integer_world(built):
    for name, (x, cent, xq, a) in built.items():
        best = {}
        for nprobe, k in _searches(name):
            if nprobe not in best:              # the oracle's top 128 once: its first k columns are its top k
                best[nprobe] = ivf_oracle.search(xq, x, a, cent, nprobe, 128)
            Do, Io = best[nprobe][0][:, :k], best[nprobe][1][:, :k]
            Dm, Im = ivf_oracle.model_search(xq, x, a, cent, nprobe, k)
            np.testing.assert_array_equal(Im, Io, err_msg=f"{name} nprobe {nprobe} k {k}")
            np.testing.assert_array_equal(Dm, Do, err_msg=f"{name} nprobe {nprobe} k {k}")
            if name in ("line-plateau-640", "line-mixed-385", "line-random-4097", "chunks-random"):   # another schedule
                Dm, Im = ivf_oracle.model_search(xq, x, a, cent, nprobe, k, reverse_steps=True)
                np.testing.assert_array_equal(Im, Io, err_msg=f"{name} nprobe {nprobe} k {k} reversed")
                np.testing.assert_array_equal(Dm, Do, err_msg=f"{name} nprobe {nprobe} k {k} reversed")
    x, cent, xq = ivf_oracle.nonfinite_world()
    a = np.concatenate([np.repeat(np.arange(4), [40, 60, 60, 60]), [0, 0, 0]])
    for nprobe in (1, 4):
        Do, Io = ivf_oracle.search(xq, x, a, cent, nprobe, 80)
        Dm, Im = ivf_oracle.model_search(xq, x, a, cent, nprobe, 80)
        np.testing.assert_array_equal(Im, Io)
        np.testing.assert_array_equal(Dm, Do)
        assert (Io < 220).all()
        Df, If = ivf_oracle.search(xq, x[:220], a[:220], cent, nprobe, 80)
        np.testing.assert_array_equal(Io, If)
        np.testing.assert_array_equal(Do, Df)
        if nprobe == 1:
            assert (Io[:8, :40] >= 0).all() and (Io[:8, 40:] == -1).all()      # aimed at list 0: its 40 finite rows


# where each defect shows: (world, nprobe, k), the first that the matrix below found among the new worlds
DEFECT_SHOWS_IN = {
    "drop_left_out": ("line-ascending-385", 1, 128),
    "strict_tau": ("line-plateau-640", 1, 128),          # (under the schedule that appends a step in descending row order)
    "cut_keeps_k_minus_1": ("line-descending-257", 1, 5),
    "refuse_at_255": ("line-ascending-385", 1, 128),
    "clamped_tail": ("line-ascending-33", 1, 5),
    "skip_first_of_batch": ("merge-last", 64, 128),
    "ge_kth": ("coarse-257", 1, 128),
}


def _differs(world, nprobe, k, defect):
    x, cent, xq, a = world
    Do, Io = ivf_oracle.search(xq, x, a, cent, nprobe, k)
    kind = {"scan_defect": defect} if defect in ivf_oracle.SCAN_DEFECTS else {"merge_defect": defect}
    Dm, Im = ivf_oracle.model_search(xq, x, a, cent, nprobe, k, reverse_steps=defect == "strict_tau", **kind)
    return not (np.array_equal(Im, Io) and np.array_equal(Dm, Do))


def test_every_defect_changes_the_result_of_a_new_world(built):
    assert set(DEFECT_SHOWS_IN) == set(ivf_oracle.SCAN_DEFECTS + ivf_oracle.MERGE_DEFECTS)
    for defect, (name, nprobe, k) in DEFECT_SHOWS_IN.items():
        assert _differs(built[name], nprobe, k, defect), f"defect {defect} does not show in world {name} (nprobe {nprobe}, k {k})"
    # what the bit-for-bit world of tests/test_ivf_gpu.py (1500 rows in random order, nlist 16) catches of them: printed,
    # not asserted -- the difference to the line above is what the new worlds add
    rng = np.random.default_rng(11)
    x = rng.integers(0, 5, (1500, 128)).astype(np.float16)
    x[:75] *= 0
    cent = rng.integers(0, 4, (16, 128)).astype(np.float32)
    cent[3], cent[9] = -1, -2
    xq = rng.integers(-3, 5, (2032, 128)).astype(np.float16)[:128]
    old = (x, cent, xq, ivf_oracle.assign(x, cent))
    caught = [d for d in DEFECT_SHOWS_IN if any(_differs(old, nprobe, k, d) for nprobe in (1, 16) for k in (5, 128))]
    print("defects the old exact world (first 128 queries, nprobe 1 and 16, k 5 and 128) also catches:", caught or "none",
          "-- not:", [d for d in DEFECT_SHOWS_IN if d not in caught])
