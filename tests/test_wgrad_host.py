"""What of the weight-gradient kernel can be checked without a GPU: the C ABI carries the new symbols, the split plan
(proqa_linear_wgrad_plan, a pure host function) behaves as proqa_hip.h says, and the REFERENCE_ERROR table of
tests/test_wgrad_gpu.py reproduces from tests/wgrad_oracle.py."""
import ctypes
import os

import pytest

import wgrad_oracle as oracle
from proqa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 32          # the kernel's contraction step, tokens (proqa_hip.h)


def plan(T, N, K, n_cus):
    lib = _lib.load()
    splits, ws = ctypes.c_int(-1), ctypes.c_size_t(12345)
    status = lib.proqa_linear_wgrad_plan(T, N, K, n_cus, ctypes.byref(splits), ctypes.byref(ws))
    return status, splits.value, ws.value


def test_the_symbols_are_in_the_header_and_in_the_table():
    header = open(os.path.join(ROOT, "include", "proqa_hip.h")).read()
    for name in ("proqa_linear_wgrad_f16", "proqa_linear_wgrad_plan"):
        assert f"int {name}(" in header
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert "#define PROQA_ABI_VERSION 7" in header and _lib.load().proqa_abi_version() == 7


PLAN_SHAPES = sorted(set(oracle.GAUSSIAN_CASES) | set(oracle.EXACT_CASES)
                     | {(T, N, K) for T in oracle.BERT_BASE_TOKENS for (N, K) in oracle.BERT_BASE_SHAPES})


@pytest.mark.parametrize("n_cus", [256, 8])
def test_plan(n_cus):
    for T, N, K in PLAN_SHAPES:
        status, splits, ws = plan(T, N, K, n_cus)
        assert status == 0 and splits >= 1, (T, N, K)
        if splits == 1:
            assert ws == 0
        else:
            assert ws >= splits * N * K * 4
        steps = -(-T // STEP)
        assert splits <= max(1, steps)                    # slices are whole contraction steps, none empty
        if T <= STEP:
            assert splits == 1
        assert plan(T, N, K, n_cus) == (status, splits, ws)            # a pure function


def test_plan_splits_a_long_token_axis_under_a_small_output():
    assert plan(4096, 128, 128, 256)[1] > 1
    assert plan(0, 128, 128, 256)[:2] == (0, 1)
    for T in (1, 31, 32):
        assert plan(T, 768, 768, 256) == (0, 1, 0)


@pytest.mark.parametrize("T,N,K", [(64, 100, 128), (64, 128, 100), (64, 4, 128), (-1, 128, 128), (64, 0, 128), (64, 128, 0)])
def test_plan_refuses_bad_arguments(T, N, K):
    status, _, _ = plan(T, N, K, 256)
    assert status == -1                                   # PROQA_EINVAL
    with pytest.raises(_lib.ProqaError) as e:
        _lib.check(status)
    assert "linear_wgrad_plan" in str(e.value)


def test_the_recorded_reference_errors_reproduce():
    from test_wgrad_gpu import BOUNDS, REFERENCE_ERROR
    measured = oracle.measure_reference_error()
    assert set(measured) == set(REFERENCE_ERROR) == set(oracle.GAUSSIAN_CASES)
    for case, err in measured.items():
        print(case, f"measured {err:.4e} recorded {REFERENCE_ERROR[case]:.4e}")
        assert err <= REFERENCE_ERROR[case], case
        assert REFERENCE_ERROR[case] <= 1.01 * err + 1e-12, case         # (and the table is not padded)
        assert BOUNDS[case] == 4.0 * REFERENCE_ERROR[case]


def test_the_oracle_restates_itself():
    dy, x, dw0 = oracle.integer_inputs(65, 200, 72)
    ref = oracle.reference(dy, x, dw0)
    assert (oracle.restated_fp32(dy, x, dw0).double() == ref).all() and ref.abs().max() < 2 ** 24
    assert (oracle.restated_fp32(dy, x).double() == oracle.reference(dy, x)).all()
