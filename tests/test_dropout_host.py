"""What of the towers' dropout can be checked without a GPU: the generator of csrc/dropout_rng.h (through the library's
pure host function proqa_dropout_keep_host) against the numpy restatement of tests/dropout_oracle.py, the statistics of
the masks, the oracle against tests/train_oracle.py, the constructor's refusals, and the tolerance tables of
tests/test_dropout_gpu.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dropout_oracle as oracle
import train_oracle
from proqa_amd.retriever import random_state_dict

CFG = train_oracle.SMALL_CONFIG
L, NH = CFG["num_hidden_layers"], CFG["num_attention_heads"]
SEED, CALL = 0x9E3779B97F4A7C15, 0x012345
HIDDEN, PROBS = 0, 1


def test_philox_known_answers():
    """Random123's known-answer vectors of Philox4x32-10"""
    hexes = lambda words: " ".join(f"{int(w):08x}" for w in words)
    assert hexes(oracle.philox4x32_10(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert hexes(oracle.philox4x32_10(f, f, f, f, f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_threshold_and_factor():
    assert oracle.threshold(0.1) == 6554 and abs(oracle.p_eff(0.1) - 0.100006) < 1e-6
    assert oracle.threshold(0.5) == 32768 and oracle.factor(0.5) == 2.0
    assert oracle.threshold(0.0) == 0 and oracle.factor(0.0) == 1.0
    assert oracle.threshold(0.9999999) == 65535
    assert oracle.factor(0.1) == float(np.float32(1.0) / np.float32(58982.0 / 65536.0))


def host_keep(kind, p, seed, site, call, a, b, c0, n):
    from proqa_amd import _lib
    lib = _lib.load()
    keep = np.full(n, 7, dtype=np.uint8)
    _lib.check(lib.proqa_dropout_keep_host(kind, p, seed, site, call, a, b, c0, n, keep.ctypes.data))
    return keep.astype(bool)


def test_host_function_reproduces_the_known_answer():
    # counter 0, key 0, p = 0.5: the halves of 6627e8d5 e169c58d bc57ac4c 9b00dbd8, low half first, against 0x8000
    got = host_keep(HIDDEN, 0.5, 0, 0, 0, 0, 0, 0, 8)
    assert got.tolist() == [True, False, True, True, True, True, True, True]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows,cols", [(1, 128), (37, 128), (300, 768)])
def test_hidden_masks_of_the_library_equal_the_oracle(rows, cols, p):
    site = oracle.site_of(1, 1)
    want = oracle.hidden_mask(p, SEED, site, CALL, rows, cols)
    got = np.stack([host_keep(HIDDEN, p, SEED, site, CALL, r, 0, 0, cols) for r in range(rows)])
    assert np.array_equal(got, want)
    # a run that starts inside a group of eight
    assert np.array_equal(host_keep(HIDDEN, p, SEED, site, CALL, rows - 1, 0, 5, cols - 5), want[rows - 1, 5:])


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n_heads", [2, 12])
@pytest.mark.parametrize("lens", [[17, 64, 65, 128, 129, 3], [200, 512, 1]])
def test_attention_masks_of_the_library_equal_the_oracle(lens, n_heads, p):
    site = oracle.site_of(1, 0)
    masks = oracle.attention_masks(p, SEED, site, CALL, lens, n_heads)
    heads = range(n_heads) if n_heads == 2 else (0, 5, 11)          # (12 heads: the first, one inside, the last)
    for b, n in enumerate(lens):
        for h in heads:
            pair = b * n_heads + h
            got = np.stack([host_keep(PROBS, p, SEED, site, CALL, pair, i, 0, n) for i in range(n)])
            assert np.array_equal(got, masks[b][h].numpy()), (b, h)
    n = lens[0]
    assert np.array_equal(host_keep(PROBS, p, SEED, site, CALL, 1, n - 1, 3, n - 3), masks[0][1].numpy()[n - 1, 3:])


def test_host_function_refuses_bad_arguments():
    from proqa_amd import _lib
    lib = _lib.load()
    keep = np.zeros(8, dtype=np.uint8)
    call = lambda kind, p, site, a=0, n=8: lib.proqa_dropout_keep_host(kind, p, 1, site, 0, a, 0, 0, n, keep.ctypes.data)
    assert call(HIDDEN, 0.1, 0) == 0
    assert call(2, 0.1, 0) == -1 and call(HIDDEN, 1.0, 0) == -1 and call(HIDDEN, -0.1, 0) == -1
    assert call(HIDDEN, float("nan"), 0) == -1 and call(HIDDEN, 0.1, 256) == -1 and call(HIDDEN, 0.1, 0, a=-1) == -1
    assert lib.proqa_abi_version() == 7


# ---- statistics (the oracle alone: the library's masks are its masks, above) ---------------------------------------------------

ROWS, COLS = 300, 768


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_fraction(p):
    keep = oracle.hidden_mask(p, SEED, oracle.site_of(1, 1), CALL, ROWS, COLS)
    n, rate = keep.size, oracle.p_eff(p)
    sigma = math.sqrt(rate * (1 - rate) / n)
    print("p", p, "kept", keep.mean(), "expected", 1 - rate, "sigma", sigma)
    assert abs(keep.mean() - (1 - rate)) <= 5 * sigma
    # attention masks too: every (query, key) of one long sequence
    probs = oracle.probs_mask(p, SEED, oracle.site_of(1, 0), CALL, 3, 512)
    assert abs(probs.mean() - (1 - rate)) <= 5 * math.sqrt(rate * (1 - rate) / probs.size)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_masks_of_different_calls_and_sites_are_independent(p):
    site = oracle.site_of(1, 1)
    first = oracle.hidden_mask(p, SEED, site, CALL, ROWS, COLS)
    rate = oracle.p_eff(p)
    agree = (1 - rate) ** 2 + rate ** 2
    sigma = math.sqrt(agree * (1 - agree) / first.size)
    others = {"call + 1": oracle.hidden_mask(p, SEED, site, CALL + 1, ROWS, COLS),
              "site + 1": oracle.hidden_mask(p, SEED, site + 1, CALL, ROWS, COLS),
              "seed + 1": oracle.hidden_mask(p, SEED + 1, site, CALL, ROWS, COLS),
              "seed + 2^32": oracle.hidden_mask(p, SEED + (1 << 32), site, CALL, ROWS, COLS)}
    for name, other in others.items():
        got = (first == other).mean()
        print("p", p, name, "agree on", got, "expected", agree, "sigma", sigma)
        assert abs(got - agree) <= 5 * sigma, name
    # the call wraps at 24 bits and shares its counter word with the site
    assert np.array_equal(first, oracle.hidden_mask(p, SEED, site, CALL + (1 << 24), ROWS, COLS))


# ---- the oracle with nothing dropped is tests/train_oracle.py ------------------------------------------------------------------

def test_all_ones_masks_give_the_operators_of_train_oracle():
    g = torch.Generator().manual_seed(3)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    x, bias, res, gamma, beta, dy = r(9, 128), r(128), r(9, 128), r(128), r(128), r(9, 128)
    ones = torch.ones(9, 128, dtype=torch.float64)
    assert torch.equal(oracle.bias_residual_layernorm_dropout_forward(x, bias, res, gamma, beta, 1e-12, ones),
                       train_oracle.bias_residual_layernorm_forward(x, bias, res, gamma, beta, 1e-12))
    got = oracle.bias_residual_layernorm_dropout_backward(dy, x, bias, res, gamma, 1e-12, ones)
    want = train_oracle.bias_residual_layernorm_backward(dy, x, bias, res, gamma, 1e-12)
    assert torch.equal(got["dx"], want["dz"]) and torch.equal(got["dresidual"], want["dz"])
    assert all(torch.equal(got[k], want[k]) for k in ("dgamma", "dbeta", "dbias"))
    lens, nh = [5, 70, 1], 2
    qkv, qb, d_ctx = r(76, 384), r(384), r(76, 128)
    Ds = [torch.ones(nh, n, n, dtype=torch.float64) for n in lens]
    for b in (qb, None):
        got = oracle.attention_dropout_forward(qkv, b, lens, nh, Ds)
        want = train_oracle.attention_forward(qkv, b, lens, nh)
        assert (got - want).abs().max() < 1e-13                    # (the value bias times a row sum of 1 +- 1 ulp)
        got = oracle.attention_dropout_backward(qkv, b, d_ctx, lens, nh, Ds)["d_qkv"]
        assert (got - train_oracle.attention_backward(qkv, b, d_ctx, lens, nh)["d_qkv"]).abs().max() < 1e-12


def test_rate_zero_gives_the_tower_of_train_oracle():
    sd = {k: v.double() for k, v in random_state_dict(CFG, seed=0).items()}
    batch = train_oracle.small_batch(0)
    got = oracle.model_forward(sd, batch, L, NH, 0.0, 0.0, 0, 0)
    want = train_oracle.model_forward(sd, batch, L, NH)
    assert all((got[k] - want[k]).abs().max() < 1e-12 for k in ("q", "c"))
    dropped = oracle.model_forward(sd, batch, L, NH, 0.1, 0.1, 0, 0)
    assert (dropped["q"] - want["q"]).abs().max() > 1e-3


def test_value_bias_does_not_drop_out_under_dropout():
    """The trap of the change: with dropped probabilities the gradient of qkv depends on the value bias."""
    import test_dropout_gpu as T
    c, Ds, _, ref = T.attention_case(2, "ragged", True, 4.0, 0.1)
    no_bv = c["bias"].clone()
    no_bv[256:] = 0
    other = oracle.attention_dropout_backward(c["qkv"], no_bv, c["d_ctx"], c["lens"], 2, Ds)
    assert oracle.rel_err(other["d_qkv"], ref["d_qkv"]) > 0.5


# ---- the constructor ---------------------------------------------------------------------------------------------------------------

def test_constructor_refusals():
    from proqa_amd.trainable import TrainableRetriever
    with pytest.raises(ValueError, match="dropout") as e:
        TrainableRetriever(CFG, device="cuda", dropout=0.1)
    assert "hidden_dropout_prob" in str(e.value) and "attention_probs_dropout_prob" in str(e.value)
    for kw in ({"hidden_dropout_prob": 0.95}, {"hidden_dropout_prob": -0.1}, {"attention_probs_dropout_prob": 1.0},
               {"attention_probs_dropout_prob": float("nan")}):
        with pytest.raises(ValueError, match="dropout"):
            TrainableRetriever(CFG, device="cuda", **kw)
    with pytest.raises(TypeError):
        TrainableRetriever(CFG, "cuda", 0.0, 0.1)                   # the rates are keyword-only
    with pytest.raises(RuntimeError, match="no CPU path"):
        TrainableRetriever(CFG, device="cpu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)


# ---- the tolerance tables of tests/test_dropout_gpu.py -------------------------------------------------------------------------------

def test_measure_reference_error_reproduces_the_tolerance_tables():
    """Summation order inside torch's CPU kernels may move the figures a little between machines; the GPU tests use the
    recorded figures, this test says when they have drifted."""
    import test_dropout_gpu as T
    worst = T.measure_reference_error()
    print({op: {k: f"{v:.3e}" for k, v in d.items()} for op, d in worst.items()})
    for op, d in T.REFERENCE_ERROR.items():
        for k, recorded in d.items():
            assert worst[op][k] == pytest.approx(recorded, rel=0.25), (op, k, worst[op][k], recorded)
            assert f"{recorded:.3e}" in T.__doc__ and f"{4 * recorded:.3e}" in T.__doc__, (op, k)
    module = T.measure_module_reference_error()
    print({k: f"{v:.3e}" for k, v in module.items()})
    assert set(module) == set(T.MODULE_REFERENCE_ERROR)
    for k, recorded in T.MODULE_REFERENCE_ERROR.items():
        assert module[k] == pytest.approx(recorded, rel=0.25), (k, module[k], recorded)
        assert f"{recorded:.3e}" in T.__doc__ and f"{4 * recorded:.3e}" in T.__doc__, k


def test_restatement_fits_the_fixed_batch_with_dropout():
    """The training condition of tests/test_dropout_gpu.py on the fp32 restatement with the module's masks"""
    import test_dropout_gpu as T
    got = T.measure_train_restatement()
    print(got)
    for seed, (loss, correct) in got.items():
        assert correct == 8
        assert loss == pytest.approx(T.TRAIN_RESTATEMENT_LOSS[seed], rel=0.5, abs=1e-4), (seed, loss)
    assert T.TRAIN_LOSS_BOUND == max(0.2, 4 * max(T.TRAIN_RESTATEMENT_LOSS.values()))
