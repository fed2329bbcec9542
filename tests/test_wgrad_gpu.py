"""proqa_linear_wgrad_f16 on the GPU against tests/wgrad_oracle.py, and the weight gradients of TrainableRetriever that
now come from it.

Shapes: T in {1, 7, 64, 65, 300, 1027, 4096} with (N, K) = (128, 128) and (200, 72) (the edge-tile case), and every
(N, K) of {(128, 128), (384, 128), (512, 128), (128, 512), (200, 72), (768, 768)} with T = 300 and 1027: one and several
tiles, one and several slices of the token axis (asserted through the plan), a last contraction step that is full, one row
long and anything between.

Tolerances
  Gaussian   seeded N(0, 1) fp16 inputs; max|gpu - ref| / max|ref| against float64.  The bound is four times the same
             measure of wgrad_oracle.restated_fp32 (an fp32 running sum in ascending t, the reference's own arithmetic
             with fp32 master gradients), measured on the CPU per case (tests/test_wgrad_host.py keeps the table
             honest); the factor 4 is the one DESIGN sections 3d / 3e give device intrinsics and re-associated sums.
             measured / allowed:
                 T = 1     (128, 128) 0         / 0            (200, 72) 0         / 0
                 T = 7     (128, 128) 7.254e-08 / 2.902e-07    (200, 72) 8.711e-08 / 3.484e-07
                 T = 64    (128, 128) 3.083e-07 / 1.233e-06    (200, 72) 2.357e-07 / 9.428e-07
                 T = 65    (128, 128) 2.901e-07 / 1.160e-06    (200, 72) 2.420e-07 / 9.680e-07
                 T = 300   (128, 128) 6.400e-07 / 2.560e-06    (200, 72) 5.264e-07 / 2.106e-06
                           (384, 128) 5.827e-07 / 2.331e-06    (512, 128) 6.793e-07 / 2.717e-06
                           (128, 512) 5.658e-07 / 2.263e-06    (768, 768) 7.393e-07 / 2.957e-06
                 T = 1027  (128, 128) 1.003e-06 / 4.012e-06    (200, 72) 1.027e-06 / 4.108e-06
                           (384, 128) 1.213e-06 / 4.852e-06    (512, 128) 1.377e-06 / 5.508e-06
                           (128, 512) 1.006e-06 / 4.024e-06    (768, 768) 1.341e-06 / 5.364e-06
                 T = 4096  (128, 128) 2.341e-06 / 9.364e-06    (200, 72) 2.068e-06 / 8.272e-06
  exact      integer-valued inputs in [-8, 8]: every partial sum is below 2^24, so the fp32 result equals the float64 one
             bit for bit, with and without accumulation onto an integer-valued dw.
  module     the whole-module bounds of tests/test_trainable_gpu.py, imported, not copied.
"""
import ctypes
import functools

import pytest
import torch

import wgrad_oracle as oracle

pytestmark = pytest.mark.gpu

REFERENCE_ERROR = {
    (1, 128, 128): 0.0,
    (7, 128, 128): 7.254e-08,
    (64, 128, 128): 3.083e-07,
    (65, 128, 128): 2.901e-07,
    (300, 128, 128): 6.400e-07,
    (1027, 128, 128): 1.003e-06,
    (4096, 128, 128): 2.341e-06,
    (1, 200, 72): 0.0,
    (7, 200, 72): 8.711e-08,
    (64, 200, 72): 2.357e-07,
    (65, 200, 72): 2.420e-07,
    (300, 200, 72): 5.264e-07,
    (1027, 200, 72): 1.027e-06,
    (4096, 200, 72): 2.068e-06,
    (300, 384, 128): 5.827e-07,
    (300, 512, 128): 6.793e-07,
    (300, 128, 512): 5.658e-07,
    (300, 768, 768): 7.393e-07,
    (1027, 384, 128): 1.213e-06,
    (1027, 512, 128): 1.377e-06,
    (1027, 128, 512): 1.006e-06,
    (1027, 768, 768): 1.341e-06,
}
BOUNDS = {k: 4.0 * v for k, v in REFERENCE_ERROR.items()}


def splits_of(dev, T, N, K):
    from proqa_amd import _lib
    splits, ws = ctypes.c_int(0), ctypes.c_size_t(0)
    n_cus = torch.cuda.get_device_properties(dev).multi_processor_count
    _lib.check(_lib.load().proqa_linear_wgrad_plan(T, N, K, n_cus, ctypes.byref(splits), ctypes.byref(ws)))
    return splits.value


def wgrad(dev, dy, x, out=None, accumulate=False):
    from proqa_amd.trainable import linear_wgrad
    got = linear_wgrad(dy.to(dev), x.to(dev), out=out, accumulate=accumulate)
    assert got.dtype == torch.float32 and got.shape == (dy.shape[1], x.shape[1]) and got.is_contiguous()
    return got


def poison_workspace(dev):
    """fill the operators' scratch with NaN, as a previous user might have left it"""
    from proqa_amd import trainable
    ws = trainable._workspace(dev, 64 << 20)
    ws.view(torch.float32).fill_(float("nan"))


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_the_cases_cover_one_slice_and_several(gpu_device):
    splits = {c: splits_of(gpu_device, *c) for c in oracle.GAUSSIAN_CASES}
    print(splits)
    assert any(s == 1 for s in splits.values()) and any(s > 1 for s in splits.values())
    assert splits[(4096, 128, 128)] > 1 and splits[(1, 128, 128)] == 1
    assert any(splits[c] > 1 for c in oracle.EXACT_CASES) and any(splits[c] == 1 for c in oracle.EXACT_CASES)


@pytest.mark.parametrize("T,N,K", oracle.GAUSSIAN_CASES)
def test_gaussian_inputs_against_float64(gpu_device, T, N, K):
    dy, x = oracle.gaussian_inputs(T, N, K)
    got = wgrad(gpu_device, dy, x).cpu()
    err, bound = oracle.rel_err(got, oracle.gaussian_reference(T, N, K)), BOUNDS[(T, N, K)]
    print(f"T={T} N={N} K={K} splits={splits_of(gpu_device, T, N, K)}: error {err:.3e} bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("T,N,K", oracle.EXACT_CASES)
def test_integer_inputs_are_exact(gpu_device, T, N, K):
    dy, x, dw0 = oracle.integer_inputs(T, N, K)
    want = oracle.reference(dy, x)
    got = wgrad(gpu_device, dy, x).cpu()
    assert (got.double() == want).all(), (got.double() - want).abs().max()
    acc = dw0.to(gpu_device).clone()
    assert wgrad(gpu_device, dy, x, out=acc, accumulate=True) is acc
    assert (acc.cpu().double() == oracle.reference(dy, x, dw0)).all()
    # out= without accumulate overwrites whatever was there
    acc.fill_(float("nan"))
    wgrad(gpu_device, dy, x, out=acc)
    assert (acc.cpu().double() == want).all()


def test_no_tokens(gpu_device):
    _, _, dw0 = oracle.integer_inputs(65, 200, 72)
    dy, x = torch.empty((0, 200), dtype=torch.float16), torch.empty((0, 72), dtype=torch.float16)
    acc = dw0.to(gpu_device).clone()
    wgrad(gpu_device, dy, x, out=acc, accumulate=True)
    assert same_bits(acc.cpu(), dw0)
    assert (wgrad(gpu_device, dy, x, out=acc).cpu() == 0).all()
    assert (wgrad(gpu_device, dy, x).cpu() == 0).all()


def test_range_where_the_fp16_product_overflows(gpu_device):
    T, N, K = 4096, 128, 128
    dy, x = torch.full((T, N), 16.0, dtype=torch.float16), torch.full((T, K), 16.0, dtype=torch.float16)
    got = wgrad(gpu_device, dy, x).cpu()
    assert (got == 1048576.0).all()
    replaced = (dy.to(gpu_device).t() @ x.to(gpu_device)).float().cpu()       # what the module ran before: fp16 out
    assert torch.isinf(replaced).all()


@pytest.mark.parametrize("T,N,K", [(65, 200, 72), (1027, 128, 128), (1027, 768, 768)])
def test_two_runs_same_bits_whatever_the_workspace_held(gpu_device, T, N, K):
    dy, x = (t.to(gpu_device) for t in oracle.gaussian_inputs(T, N, K))
    first = wgrad(gpu_device, dy, x).cpu()
    poison_workspace(gpu_device)
    second = wgrad(gpu_device, dy, x).cpu()
    assert torch.isfinite(second).all() and same_bits(first, second)


@pytest.mark.parametrize("T,N,K", [(65, 200, 72), (1027, 128, 128)])
def test_non_finite_inputs_stay_in_their_row_and_column(gpu_device, T, N, K):
    dy, x = oracle.gaussian_inputs(T, N, K)
    clean = wgrad(gpu_device, dy, x).cpu()
    t0, n0, k0 = T - 3, N - 5, K - 7
    bad = dy.clone()
    bad[t0, n0] = float("inf")
    got = wgrad(gpu_device, bad, x).cpu()
    assert not torch.isfinite(got[n0]).any()
    rest = torch.arange(N) != n0
    assert same_bits(got[rest], clean[rest])
    bad = x.clone()
    bad[t0, k0] = float("nan")
    got = wgrad(gpu_device, dy, bad).cpu()
    assert not torch.isfinite(got[:, k0]).any()
    rest = torch.arange(K) != k0
    assert same_bits(got[:, rest].contiguous(), clean[:, rest].contiguous())


@pytest.mark.parametrize("T,N,K", [(65, 200, 72), (1027, 128, 128)])
def test_linear_in_dy(gpu_device, T, N, K):
    dy, x = oracle.gaussian_inputs(T, N, K)
    assert dy.abs().max() * 1024.0 < 65504.0               # dy * 1024 stays finite in fp16
    one = wgrad(gpu_device, dy, x).cpu()
    scaled = wgrad(gpu_device, dy * 1024.0, x).cpu()
    assert torch.isfinite(scaled).all() and same_bits(scaled, one * 1024.0)


def test_bad_arguments(gpu_device):
    from proqa_amd import _lib
    from proqa_amd.trainable import linear_wgrad
    dy = torch.zeros((16, 128), dtype=torch.float16, device=gpu_device)
    with pytest.raises(_lib.ProqaError, match="multiples of 8"):
        linear_wgrad(dy, torch.zeros((16, 100), dtype=torch.float16, device=gpu_device))
    with pytest.raises(ValueError):
        linear_wgrad(dy, torch.zeros((15, 128), dtype=torch.float16, device=gpu_device))
    with pytest.raises(ValueError):
        linear_wgrad(dy, dy, out=torch.zeros((128, 128), dtype=torch.float16, device=gpu_device))
    with pytest.raises(ValueError):
        linear_wgrad(dy, dy, accumulate=True)


# ---- the module ---------------------------------------------------------------------------------------------------------

def is_weight_matrix(key):
    return key.endswith(".weight") and ("encoder.layer" in key or "pooler" in key or key.startswith("proj_")) \
        and "LayerNorm" not in key


@functools.lru_cache(maxsize=None)
def module_backward(dev):
    """(model, {name: a copy of its gradient at loss scale 1024}) of one backward pass -- computed once"""
    from proqa_amd.trainable import inbatch_loss
    from test_trainable_gpu import LOSS_SCALE, make_model, on, reference
    sd, batch, *_ = reference()
    model = make_model(dev, sd)
    out = model(on(dev, batch))
    (inbatch_loss(out["q"], out["c"]) * LOSS_SCALE).backward()
    return model, {k: p.grad.clone() for k, p in model.named_parameters()}


def test_module_weight_gradients_are_fp32_sums_within_the_module_bounds(gpu_device):
    import train_oracle
    from test_trainable_gpu import BOUNDS as MODULE_BOUNDS, LOSS_SCALE, kind, reference
    _, _, _, ref, _ = reference()
    _, grads = module_backward(gpu_device)
    weights = [k for k in grads if is_weight_matrix(k)]
    assert len(weights) == 2 * (6 * 2 + 1) + 2             # per tower: 6 matrices in each of 2 layers and the pooler; 2 projections
    for k in weights:
        g = grads[k]
        assert g.dim() == 2 and g.dtype == torch.float32
        err, bound = train_oracle.rel_err(g.detach().cpu().double() / LOSS_SCALE, ref[k]), MODULE_BOUNDS[kind(k)]
        not_fp16 = (g.half().float() != g).float().mean().item()
        print(f"{k}: error {err:.3e} bound {bound:.3e}; {not_fp16:.3f} of the elements are not fp16 numbers")
        assert err <= bound
        assert not_fp16 > 0.5


def test_module_backward_twice_same_bits_then_a_fused_step_without_a_sync(gpu_device):
    from proqa_amd.optim import FusedAdamW
    from proqa_amd.trainable import inbatch_loss
    from test_trainable_gpu import LOSS_SCALE, on, reference
    _, batch, *_ = reference()
    model, first = module_backward(gpu_device)
    model.zero_grad()
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_grad_norm=2.0, loss_scale=LOSS_SCALE, torch_semantics=True)
    opt.step()                                               # (first use: pinned staging memory is allocated; no gradients)
    poison_workspace(gpu_device)
    out = model(on(gpu_device, batch))
    opt.scale_loss(inbatch_loss(out["q"], out["c"])).backward()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    for k, p in model.named_parameters():
        if is_weight_matrix(k):
            assert same_bits(p.grad, first[k]), k
            assert p.grad.is_contiguous() and p.grad.data_ptr() % 16 == 0 and p.grad.dtype == torch.float32, k
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert opt.state_dict()["fused"]["skipped_steps"] == 0
    for k, p in model.named_parameters():
        if is_weight_matrix(k):
            assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[k]), k
