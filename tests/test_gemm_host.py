"""The yardstick of tests/test_gemm_gpu.py, checked without a GPU: the recorded reference ratio reproduces, the float32
restatement of proqa_gemm_tn_f16 passes its bound on every case, family and epilogue of the GPU test's list, each mutant of
the restatement -- the errors of the tile walk, the ring and the epilogue the tests are meant to catch -- fails on at least
one listed case, and the model of the tile walk visits every tile exactly once and reaches every path it names."""
import numpy as np
import pytest

import gemm_oracle as G

O = G.O


def test_the_recorded_reference_ratio_reproduces():
    measured = G.measure_reference_error()
    assert set(measured) == set(G.REFERENCE_RATIO)
    for op, r in measured.items():
        print(f"{op:10s} measured {r:.4f}   recorded {G.REFERENCE_RATIO[op]:.4f}")
        # the BLAS' float32 summation order is the machine's: a tenth either way, and the table is not padded
        assert r <= 1.1 * G.REFERENCE_RATIO[op], op
        assert G.REFERENCE_RATIO[op] <= 1.25 * r, op
    assert G.GAMMA_GEMM == 4.0 * G.REFERENCE_RATIO["gemm"] and G.GAMMA_GELU == O.GAMMA["gelu"] and G.FIT == 4.6e-5
    assert measured["gelu_erf4"] <= G.GAMMA_GELU            # the restated GELU needs no more than FIT and the GELU units


@pytest.fixture(scope="module")
def survey():
    """One pass over the case list: outputs of the restatement outside the bound per (case, family, epilogue), and per
    (mutant, case) on the int family -- epilogue 1 compared exactly as the GPU test does (epilogue 2 under its bound for
    the mutant that exists only there)."""
    clean, mutants, int_range = {}, {}, {}
    for case in G.CASES:
        for family in G.FAMILIES:
            x, w, bias = G.inputs(*case, family)
            ref = G.GemmRef(x, w, bias)
            exact = family in ("int", "overflow")
            for epi in (0, 1, 2):
                with np.errstate(over="ignore"):
                    got = O.h16(G.gemm_f32(x, w, bias, epi))
                clean[case, family, epi] = int(ref.outside(got, epi).sum())
                if exact and epi < 2:
                    assert (G.gemm_f32(x, w, bias, epi) == ref.pre(epi)).all(), (case, family, epi)
            if family == "overflow":
                with np.errstate(over="ignore"):
                    int_range[case, family] = float(np.isinf(O.h16(ref.pre(1))).mean())
            if family != "int":
                continue
            int_range[case, family] = float(np.abs(ref.pre(1)).max())
            for mutant in G.GEMM_MUTANTS:
                if mutant == "gelu_before_bias":
                    bad = int(ref.outside(O.h16(G.gemm_f32(x, w, bias, 2, mutant=mutant)), 2).sum())
                else:
                    bad = int((~(O.f64(O.h16(G.gemm_f32(x, w, bias, 1, mutant=mutant))) == ref.pre(1))).sum())
                mutants[mutant, case] = bad
    return clean, mutants, int_range


def test_the_restatement_misses_no_bound(survey):
    clean, _, _ = survey
    assert len(clean) == len(G.CASES) * len(G.FAMILIES) * 3
    assert not {k: v for k, v in clean.items() if v}


def test_the_families_are_what_they_say(survey):
    _, _, int_range = survey
    for case in G.CASES:
        assert int_range[case, "int"] <= 2048, case                  # integers that fp16 holds exactly
        assert 0.005 < int_range[case, "overflow"] < 0.2, case       # some pre-activations beyond +-65504, most not
        x, w, bias = G.inputs(*case, "subnormal")
        assert 0 < np.abs(O.f64(x)).min() and np.abs(O.f64(x)).max() < 2.0 ** -14
        ref = G.GemmRef(x, w, bias)
        assert np.median(np.abs(ref.pre(0))) > 2.0 ** -10           # flushed operands would give zeros: far outside the bound
        assert ref.outside(np.zeros_like(ref.pre(0)), 0).mean() > 0.9
    bias = G.feature_pattern(2816)
    n = np.arange(2816 - 256)
    assert (bias[n] != bias[n + 1]).all() and (bias[n] != bias[n + 256]).all()
    assert (bias[n] != bias[n + 8])[(n % 256) < 248].all()


@pytest.mark.parametrize("mutant", G.GEMM_MUTANTS)
def test_each_mutant_of_the_product_fails_somewhere(survey, mutant):
    _, mutants, _ = survey
    caught = {case: bad for (m, case), bad in mutants.items() if m == mutant and bad}
    print(mutant, caught)
    assert caught
    if mutant == "stale_ring_buffer":                        # two K-steps have no step s - 2
        assert set(caught) == {c for c in G.CASES if c[2] >= 192}
    elif mutant == "neighbour_tile_bias":
        assert set(caught) == {c for c in G.CASES if c[1] > 256}
    elif mutant == "slabs_exchanged":
        assert set(caught) == {c for c in G.CASES if c[0] > 256}
    else:
        assert set(caught) == set(G.CASES)


def test_gelu_on_every_fp16_argument_and_its_mutants():
    """The restated gelu_erf4 misses no bound with the documented fit error granted and some without it; it is never more than
    one fp16 step from the correctly rounded result; the tanh form, a clamp at 4 and a fit twice as far off all fail."""
    for zero_bias in (False, True):
        x, w, bias = G.every_fp16_inputs(zero_bias)
        ref = G.EveryFp16Ref(x, w, bias)
        assert len(set(x.reshape(-1)[:63488].view(np.uint16).tolist())) == 63488 and np.isfinite(x).all() and not x.reshape(-1)[63488:].any()
        with np.errstate(over="ignore"):
            got = [O.h16(G.gemm_f32(x, w, bias, epi)) for epi in (0, 1, 2)]
            for epi in (0, 1, 2):
                assert ref.outside(got[epi], epi).sum() == 0, (zero_bias, epi)
            assert (O.f64(got[0])[:, :64] == O.f64(x)).all()          # (-0 comes back as +0: compared as values)
            steps = G.ulps_off(got[2], ref.out(2))
            without_fit = O.gelu_mismatches(got[2], ref.x, np.broadcast_to(bias, ref.x.shape))
            print(f"zero_bias={zero_bias}: {100 * (steps > 0).mean():.2f} % of the outputs one step off the correctly rounded "
                  f"result; {int(without_fit.sum())} outside the bound without the FIT term")
            assert steps.max() == 1 and without_fit.sum() > 0
            for mutant in G.GELU_MUTANTS:
                bad = int(ref.outside(O.h16(G.gemm_f32(x, w, bias, 2, gelu_mutant=mutant)), 2).sum())
                print(f"    {mutant}: {bad} of {steps.size} outside")
                assert bad > 0, mutant


# ---- the tile walk ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cus", G.CU_COUNTS)
def test_the_walk_visits_every_tile_exactly_once(n_cus):
    for case in G.CASES + (G.EVERY_FP16_SHAPE, (65536, 3072, 768), (16384, 768, 3072), (7936, 768, 768)):
        assert (G.visits(*case, n_cus) == 1).all(), (case, n_cus)
        assert len(G.schedule_model(*case, n_cus)) == min(case[0] // 256 * (case[1] // 256), n_cus)     # the floor changes nothing here


def test_the_case_list_reaches_every_path_at_256_cus():
    per_case = {case: G.path_labels(*case, 256) for case in G.CASES}
    for case, labels in per_case.items():
        print(case, sorted(labels))
    assert G.labels_reached(256) == set(G.PATH_LABELS)
    assert {"two_slabs_and_ragged_group", "idle_workgroup", "one_tile_workgroup", "several_tile_workgroup"} <= per_case[2304, 2304, 192]
    assert per_case[256, 256, 64] == {"k_steps_1", "one_tile_workgroup"}
    for n_cus in G.CU_COUNTS:                                # elsewhere only the capped grid may be out of reach
        assert set(G.PATH_LABELS) - G.labels_reached(n_cus) <= {"grid_capped"}, n_cus


@pytest.mark.parametrize("n_cus", range(1, 8))
def test_fewer_than_8_cus_need_the_grid_floor(n_cus):
    holes = {case: int((G.visits(*case, n_cus, floor=False) == 0).sum()) for case in G.CASES}
    print(n_cus, holes)
    assert holes[2304, 2304, 192] > 0 and holes[8448, 2048, 64] > 0
    assert all((G.visits(*case, n_cus, floor=False) <= 1).all() for case in G.CASES)
    for case in G.CASES:
        assert (G.visits(*case, n_cus) == 1).all(), case
