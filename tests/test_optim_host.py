"""What of the fused optimizer step can be checked without a GPU: the float64 restatement the GPU tests compare against
(tests/adamw_oracle.py) equals torch.optim.AdamW + clip_grad_norm_ and the reference's transformers.AdamW, the C ABI
validates its arguments before it touches a device, and the tolerance table of tests/test_optim_gpu.py reproduces."""
import ctypes
import math

import numpy as np
import pytest
import torch

import adamw_oracle as oracle
from proqa_amd import _lib

SHAPES = [(1,), (3,), (7,), (128,), (768,), (33, 5), (120, 128), (1000,), (2, 3, 4), (17,), (64, 64), (5,), (9, 9), (300,)]
assert len(SHAPES) == 14
WDS = [0.01 if i % 2 == 0 else 0.0 for i in range(len(SHAPES))]
LRS = [1e-3 if i % 2 == 0 else 5e-4 for i in range(len(SHAPES))]


def _tensors(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen, dtype=torch.float64) * 0.02 for s in SHAPES]


def _grads(seed, step):
    gen = torch.Generator().manual_seed(seed * 100 + step)
    return [torch.randn(s, generator=gen, dtype=torch.float64) * 0.05 for s in SHAPES]


@pytest.mark.parametrize("max_grad_norm", [None, 1.0, 1e9])
def test_float64_oracle_equals_torch_adamw_with_clipping(max_grad_norm):
    params = [torch.nn.Parameter(t.clone()) for t in _tensors(0)]
    opt = torch.optim.AdamW([{"params": params[0::2], "weight_decay": 0.01, "lr": 1e-3},
                             {"params": params[1::2], "weight_decay": 0.0, "lr": 5e-4}], betas=(0.9, 0.999), eps=1e-8)
    hp = oracle.hyper(max_grad_norm=max_grad_norm, torch_semantics=True)
    state = oracle.new_state()
    p, m, v = _tensors(0), [torch.zeros(s, dtype=torch.float64) for s in SHAPES], [torch.zeros(s, dtype=torch.float64) for s in SHAPES]
    for step in range(5):
        grads = _grads(1, step)
        for q, g in zip(params, grads):
            q.grad = g.clone()
        norm = None
        if max_grad_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(params, max_grad_norm))
        opt.step()
        state, p, m, v, info = oracle.oracle_step(state, hp, p, grads, m, v, LRS, WDS)
        if norm is not None:
            assert abs(info["norm"] - norm) <= 1e-12 * norm
            assert (info["clip"] < 1.0) == (max_grad_norm == 1.0)
        for i, q in enumerate(params):
            assert oracle.rel_err(p[i], q.detach()) < 1e-12, (step, i)
            assert oracle.rel_err(m[i], opt.state[q]["exp_avg"]) < 1e-12
            assert oracle.rel_err(v[i], opt.state[q]["exp_avg_sq"]) < 1e-12
    assert state["step"] == 5 and state["skipped_steps"] == 0


def _transformers_adamw_step(p, grad, state, group):
    """transformers.AdamW.step (optimization.py, v2-v4: the class the reference constructs with correct_bias=True), its
    per-parameter body line for line on torch tensors:

        exp_avg.mul_(beta1).add_(grad, alpha=1.0 - beta1)
        exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1.0 - beta2)
        denom = exp_avg_sq.sqrt().add_(group["eps"])
        step_size = group["lr"]
        if group["correct_bias"]:
            step_size = step_size * math.sqrt(1.0 - beta2 ** state["step"]) / (1.0 - beta1 ** state["step"])
        p.data.addcdiv_(exp_avg, denom, value=-step_size)
        if group["weight_decay"] > 0.0: p.data.add_(p.data, alpha=-group["lr"] * group["weight_decay"])
    """
    exp_avg, exp_avg_sq = state["exp_avg"], state["exp_avg_sq"]
    beta1, beta2 = group["betas"]
    state["step"] += 1
    exp_avg.mul_(beta1).add_(grad, alpha=1.0 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1.0 - beta2)
    denom = exp_avg_sq.sqrt().add_(group["eps"])
    step_size = group["lr"]
    if group["correct_bias"]:
        bias_correction1 = 1.0 - beta1 ** state["step"]
        bias_correction2 = 1.0 - beta2 ** state["step"]
        step_size = step_size * math.sqrt(bias_correction2) / bias_correction1
    p.addcdiv_(exp_avg, denom, value=-step_size)
    if group["weight_decay"] > 0.0:
        p.add_(p, alpha=-group["lr"] * group["weight_decay"])


def test_float64_oracle_equals_the_reference_optimizer():
    p_ref = _tensors(3)
    states = [{"step": 0, "exp_avg": torch.zeros_like(t), "exp_avg_sq": torch.zeros_like(t)} for t in p_ref]
    hp = oracle.hyper(torch_semantics=False)
    state = oracle.new_state()
    p, m, v = _tensors(3), [torch.zeros_like(t) for t in p_ref], [torch.zeros_like(t) for t in p_ref]
    for step in range(5):
        grads = _grads(4, step)
        for i in range(len(p_ref)):
            group = {"betas": (0.9, 0.999), "eps": 1e-8, "lr": LRS[i], "weight_decay": WDS[i], "correct_bias": True}
            _transformers_adamw_step(p_ref[i], grads[i], states[i], group)
        state, p, m, v, _ = oracle.oracle_step(state, hp, p, grads, m, v, LRS, WDS)
        for i in range(len(p_ref)):
            assert oracle.rel_err(p[i], p_ref[i]) < 1e-12 and oracle.rel_err(m[i], states[i]["exp_avg"]) < 1e-12
            assert oracle.rel_err(v[i], states[i]["exp_avg_sq"]) < 1e-12
    # the two semantics are different updates (the point of torch_semantics)
    _, p_torch, _, _, _ = oracle.oracle_step(oracle.new_state(), oracle.hyper(torch_semantics=True), _tensors(3), _grads(4, 0),
                                             [torch.zeros_like(t) for t in p_ref], [torch.zeros_like(t) for t in p_ref], LRS, WDS)
    _, p_here, _, _, _ = oracle.oracle_step(oracle.new_state(), hp, _tensors(3), _grads(4, 0),
                                            [torch.zeros_like(t) for t in p_ref], [torch.zeros_like(t) for t in p_ref], LRS, WDS)
    assert oracle.rel_err(p_here[6], p_torch[6]) > 1e-9


def test_oracle_skip_rule_and_scale_schedule():
    hp = oracle.hyper(loss_scale="dynamic", growth_interval=2, max_grad_norm=1.0)
    state = oracle.new_state("dynamic")
    p, m, v = [torch.ones(4)], [torch.zeros(4)], [torch.zeros(4)]
    bad = [torch.tensor([1.0, float("inf"), 0.0, 0.0])]
    state, p2, m2, v2, info = oracle.oracle_step(state, hp, p, bad, m, v, [1e-3], [0.0])
    assert info["found_inf"] and state == {"step": 0, "scale": 32768.0, "clean_steps": 0, "skipped_steps": 1}
    assert torch.equal(p2[0], p[0].double()) and not m2[0].any() and not v2[0].any()
    good = [torch.full((4,), 32768.0)]
    state, p2, _, _, info = oracle.oracle_step(state, hp, p, good, m, v, [1e-3], [0.0])
    assert not info["found_inf"] and abs(info["norm"] - 2.0) < 1e-12 and state["scale"] == 32768.0 and state["step"] == 1
    assert not torch.equal(p2[0], p[0].double())
    state, _, _, _, _ = oracle.oracle_step(state, hp, p, good, m, v, [1e-3], [0.0])
    assert state["scale"] == 65536.0 and state["clean_steps"] == 0 and state["step"] == 2


def test_adamw_abi_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def hyper(**kw):
        args = dict(beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0, torch_semantics=0, scale_mode=_lib.ADAMW_SCALE_DYNAMIC,
                    backoff_factor=0.5, growth_factor=2.0, growth_interval=2000, host_step=0)
        args.update(kw)
        return _lib.AdamwHyper(**args)

    def step(table=64, n_tensors=1, chunks=64, n_chunks=1, h=None, state=64, ws=64, ws_bytes=16):
        # (the addresses are never dereferenced: every call below is refused before the device is touched)
        h = hyper() if h is None else h
        return lib.proqa_adamw_step(table, n_tensors, chunks, n_chunks, ctypes.byref(h), state, ws, ws_bytes, None)

    assert step(n_tensors=-1) == -1 and b"n_tensors=-1" in lib.proqa_last_error()
    assert step(n_chunks=-1) == -1
    assert step(table=None) == -1 and b"NULL tensor table" in lib.proqa_last_error()
    assert step(chunks=None) == -1
    assert step(state=None) == -1 and b"NULL state" in lib.proqa_last_error()
    assert step(n_chunks=5, ws_bytes=16) == -1 and b"workspace too small" in lib.proqa_last_error()
    assert step(ws=None) == -1
    assert lib.proqa_adamw_step(64, 1, 64, 1, None, 64, 64, 16, None) == -1
    for bad in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(eps=-1.0), dict(scale_mode=3),
                dict(backoff_factor=1.0), dict(growth_factor=0.5), dict(growth_interval=0),
                dict(max_grad_norm=0.0, scale_mode=_lib.ADAMW_SCALE_NONE, host_step=0)):
        assert step(h=hyper(**bad)) == -1, bad
    assert b"host_step" in lib.proqa_last_error()
    assert step(h=hyper(beta1=1.0)) == -1 and b"[0, 1)" in lib.proqa_last_error()
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.proqa_adamw_state_init(64, 0, scale, 0, 0, None) == -1 and b"loss scale" in lib.proqa_last_error()
    assert lib.proqa_adamw_state_init(None, 0, 1.0, 0, 0, None) == -1
    assert lib.proqa_adamw_state_init(64, -1, 1.0, 0, 0, None) == -1
    with pytest.raises(_lib.ProqaError):
        _lib.check(step(n_tensors=-1))


def test_chunk_map_and_workspace_size():
    lib = _lib.load()
    C = _lib.ADAMW_CHUNK
    sizes = np.array([1, 0, C - 1, C, C + 1, 2 * C + 5], dtype=np.int64)
    n = lib.proqa_adamw_chunk_map(sizes.ctypes.data, len(sizes), None, 0)
    assert n == 1 + 0 + 1 + 1 + 2 + 3
    out = np.zeros((n, 2), dtype=np.int32)
    assert lib.proqa_adamw_chunk_map(sizes.ctypes.data, len(sizes), out.ctypes.data, n) == n
    assert out.tolist() == [[0, 0], [2, 0], [3, 0], [4, 0], [4, 1], [5, 0], [5, 1], [5, 2]]
    assert lib.proqa_adamw_chunk_map(sizes.ctypes.data, len(sizes), out.ctypes.data, n - 1) == -1
    assert lib.proqa_adamw_chunk_map(sizes.ctypes.data, -1, None, 0) == -1
    assert lib.proqa_adamw_chunk_map(None, 2, None, 0) == -1
    sizes[3] = -5
    assert lib.proqa_adamw_chunk_map(sizes.ctypes.data, len(sizes), None, 0) == -1
    assert lib.proqa_adamw_workspace_bytes(0) == 16 and lib.proqa_adamw_workspace_bytes(5) == 32
    assert lib.proqa_adamw_workspace_bytes(13400) >= 13400 * 4
    assert ctypes.sizeof(_lib.AdamwTensor) == 56 and ctypes.sizeof(_lib.AdamwChunk) == 8


def test_fused_adamw_refuses_what_it_cannot_take():
    from proqa_amd.optim import FusedAdamW
    with pytest.raises(ValueError, match="fp32 CUDA"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3)
    with pytest.raises(ValueError, match="betas"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="loss_scale"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, loss_scale=0.0)
    with pytest.raises(ValueError, match="loss_scale"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, loss_scale="auto")
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, max_grad_norm=0.0)


def test_measure_reference_error_reproduces_the_tolerance_table():
    """The figures in the header of tests/test_optim_gpu.py (adamw_oracle.MEASURED_FP32_ERROR): the fp32 mode of the oracle
    against its float64 mode.  Summation order inside torch's CPU kernels may move them a little between machines; the
    GPU tests use the recorded figures, this test says when they have drifted."""
    worst, per_config = oracle.measure_reference_error()
    print({k: f"{x:.3g}" for k, x in worst.items()})
    for k, recorded in oracle.MEASURED_FP32_ERROR.items():
        assert worst[k] == pytest.approx(recorded, rel=0.25), (k, worst[k], recorded)
    # the clipped runs inherit the fp32 norm's error in m and v; the others do not
    assert per_config[(None, 65536.0, False)]["m"] < 2e-7 < per_config[(1.0, 65536.0, False)]["m"]
    # the header's table is these figures
    import test_optim_gpu
    for k, recorded in oracle.MEASURED_FP32_ERROR.items():
        assert f"{recorded:.2e}" in test_optim_gpu.__doc__ and f"{4 * recorded:.2e}" in test_optim_gpu.__doc__, k
