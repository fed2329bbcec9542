"""The yardstick of tests/test_encoder_ops_gpu.py, checked without a GPU: the recorded reference ratios reproduce, the
float32 restatement of every operator passes its bound on every case of the GPU tests' lists, and each mutant of a
restatement -- the kernel errors the bounds are meant to catch -- fails its bound on at least one listed case."""
import functools

import numpy as np
import pytest

import encoder_ops_oracle as O


def n_bad(got, ref, tol, where=None):
    """Elements outside the tolerance (a NaN is outside)."""
    bad = ~(np.abs(O.f64(got) - ref) <= tol)
    return int(bad[where].sum() if where is not None else bad.sum())


def test_the_recorded_reference_ratios_reproduce():
    measured = O.measure_reference_error()
    assert set(measured) == set(O.REFERENCE_RATIO) == set(O.GAMMA)
    for op, r in measured.items():
        print(f"{op:10s} measured {r:.4f}   recorded {O.REFERENCE_RATIO[op]:.4f}   GAMMA {O.GAMMA[op]:.4f}")
        # NumPy's and the BLAS' float32 summation order is the machine's: a tenth either way, and the table is not padded
        assert r <= 1.1 * O.REFERENCE_RATIO[op], op
        assert O.REFERENCE_RATIO[op] <= 1.25 * r, op
        assert O.GAMMA[op] == 4.0 * O.REFERENCE_RATIO[op]


# ---- LayerNorm -----------------------------------------------------------------------------------------------------
def layernorm_failures(mutant):
    """{case: fraction of elements outside the bound} of the (mutated) restatement, rounded to fp16 like the kernel's store."""
    out = {}
    for key, (x, bias, res, gamma, beta, eps) in O.layernorm_cases():
        ref = O.LayerNormRef((x, bias, res), gamma, beta, eps)
        got = O.h16(O.layernorm_f32((x, bias, res), gamma, beta, eps, mutant=mutant))
        out[key] = n_bad(got, ref.out, ref.bound()) / got.size
    return out


def test_layernorm_restatement_passes_and_mutants_fail():
    assert not any(layernorm_failures(None).values())
    nm1 = layernorm_failures("n_minus_1")
    print("variance / (N - 1):", {k: round(v, 3) for k, v in nm1.items() if k[1] == 9 and k[2] == "normal"})
    assert nm1[(768, 9, "normal")] > 0.5 and nm1[(1024, 9, "normal")] > 0.3     # (6.5e-4 and 4.9e-4 relative)
    eps = layernorm_failures("eps1e-5")
    print("eps = 1e-5:", {k: round(v, 3) for k, v in eps.items() if k[1] == 9 and k[0] == 768})
    assert all(v > 0.9 for k, v in eps.items() if k[2] == "tiny_eps1e-12" and k[0] > 8)
    assert not any(v for k, v in eps.items() if k[2] == "tiny_eps1e-5")          # (that family IS eps = 1e-5)


def test_embedding_restatement_passes():
    for hidden, batch, seq_len in O.EMBED_CASES:
        c = O.embed_case(hidden, batch, seq_len)
        for typed in (False, True):
            parts = O.embed_parts(c, typed)
            ref = O.LayerNormRef(parts, c["gamma"], c["beta"], 1e-12)
            assert n_bad(O.h16(O.layernorm_f32(parts, c["gamma"], c["beta"], 1e-12)), ref.out, ref.bound()) == 0


def test_constant_rows_are_exact_in_float32():
    for cols in O.LN_COLS:
        x, bias, res, gamma, beta = O.constant_rows_case(cols, 9)
        got = O.h16(O.layernorm_f32((x, bias, res), gamma, beta, 1e-12))
        assert (got.view(np.uint16) == np.broadcast_to(beta, got.shape).view(np.uint16)).all()


# ---- GELU ----------------------------------------------------------------------------------------------------------
def test_gelu_restatement_passes_and_the_tanh_form_fails():
    for name, x, bias in O.gelu_cases():
        t32 = O.f32(x) + O.f32(bias)
        with np.errstate(over="ignore"):
            assert O.gelu_mismatches(O.h16(O.gelu_f32(t32)), x, bias).sum() == 0, name
            bad = int(O.gelu_mismatches(O.h16(O.gelu_f32(t32, mutant="tanh")), x, bias).sum())
        print(f"tanh-form GELU, {name}: {bad} of {x.size} outside the bound")
        assert bad > 1000


# ---- attention -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attention_refs():
    out = {}
    for case in O.attention_cases():
        qkv, bias = O.attention_case_inputs(case)
        out[case["name"]] = (case, qkv, bias, O.AttentionRef(qkv, bias, case["lens"], case["NH"]))
    return out


def attention_failures(mutant):
    out = {}
    for name, (case, qkv, bias, ref) in attention_refs().items():
        got = O.attention_f32(qkv, bias, case["lens"], case["NH"], mutant=mutant)
        out[name] = n_bad(got, ref.out, ref.bound(), ref.valid())
    return out


def test_attention_restatement_passes():
    assert not any(attention_failures(None).values())


@pytest.mark.parametrize("mutant", ["mask_le", "drop_last", "no_rescale_at_chunk"])
def test_attention_mutants_fail(mutant):
    bad = attention_failures(mutant)
    print(mutant, bad)
    assert bad["edges_nh1_bias0"] > 0 and bad["edges_nh2_bias1"] > 0 and bad["pairs9_S300"] > 0


def test_cls_restatement_passes_its_own_bound_and_not_the_full_kernels():
    """The [CLS] kernel reads k + b_k and v + b_v rounded to fp16.  Query 0 is planted in the even sequences only, so the
    odd ones are ordinary softmax rows: there a key bias of 40 (fp16 spacing 2^-5) moves the scores by more than the full
    kernel's bound, which has no such term, allows -- and stays inside bound_cls(), which has it."""
    lost = 0
    for name, (case, qkv, bias, ref) in attention_refs().items():
        got = O.attention_cls_f32(qkv, bias, case["lens"], case["NH"])
        assert n_bad(got, ref.out[:, :1], ref.bound_cls()) == 0, name
        lost += n_bad(O.attention_cls_f32(qkv, bias, case["lens"], case["NH"], mutant="skip_group_tail"), ref.out[:, :1], ref.bound_cls())
    assert lost > 0
    case, qkv, bias, ref = attention_refs()["key_bias40"]
    bad = n_bad(O.attention_cls_f32(qkv, bias, case["lens"], case["NH"]), ref.out[:, :1], ref.bound()[:, :1])
    print(f"[CLS] with k + 40 rounded to fp16 under the full kernel's bound: {bad} of {ref.out[:, :1].size} outside")
    assert bad > 0


def test_cls_reference_is_row_0_of_the_full_reference():
    case, qkv, bias, ref = attention_refs()["edges_nh2_bias1"]
    cls = O.AttentionRef(qkv, bias, case["lens"], case["NH"], cls_only=True)
    np.testing.assert_allclose(cls.out, ref.out[:, :1], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(cls.bound(), ref.bound()[:, :1], rtol=1e-9)
    np.testing.assert_allclose(cls.bound_cls(), ref.bound_cls(), rtol=1e-9)


def test_zero_queries_give_the_mean_of_v_and_the_key_bias_is_absent():
    case, qkv, bias, ref = attention_refs()["zero_q"]
    v = O.f64(qkv).reshape(5, 257, 3, 1, 64)[:, :, 2, 0]
    for b, n in enumerate(ref.lens):
        np.testing.assert_allclose(ref.out[b, :n], np.broadcast_to(v[b, :n].mean(0), (n, 64)), rtol=1e-13, atol=1e-15)
    case, qkv, bias, ref = attention_refs()["key_bias40"]
    other = bias.copy()
    other[128:256] = 0
    assert (O.AttentionRef(qkv, other, case["lens"], case["NH"]).out == ref.out).all()


# ---- dense and pooler ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", O.DENSE_M)
def test_dense_restatement_passes_and_a_short_k_loop_fails(M):
    for _, N, K in (c for c in O.dense_cases() if c[0] == M):
        x, w, bias = O.dense_inputs(M, N, K, "gauss")
        for act, b in ((0, None), (0, bias), (1, bias)):
            ref = O.DenseRef(x, w, b, act)
            assert n_bad(O.h16(O.dense_f32(x, w, b, act)), ref.out, ref.bound()) == 0, (M, N, K, act)
            assert n_bad(O.h16(O.dense_f32(x, w, b, act, mutant="skip_last_32k")), ref.out, ref.bound()) > 0, (M, N, K, act)
        xi, wi, bi = O.dense_inputs(M, N, K, "int")
        ref = O.DenseRef(xi, wi, bi)
        assert np.abs(ref.out).max() <= 2048 and (O.f64(O.dense_f32(xi, wi, bi)) == ref.out).all()


def test_pooler_restatement_passes():
    for hidden, batch, saturate in O.pooler_cases():
        args = O.pooler_inputs(hidden, batch, saturate=saturate)
        ref = O.PoolerRef(*args)
        if saturate:
            assert np.abs(ref.pre).max() > 12
        got = O.pooler_f32(*args)
        assert n_bad(got, ref.out, ref.bound(out32=True)) == 0
        assert n_bad(O.h16(got), ref.out, ref.bound(out32=False)) == 0
    for hidden in O.POOL_HIDDEN:
        args, expect = O.pooler_integer_inputs(hidden, 33)
        assert (O.f64(O.pooler_f32(*args)) == expect).all() and np.abs(expect).max() <= 2048
