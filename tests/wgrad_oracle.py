"""Oracle of the weight-gradient product dw[N, K] = dw0 + sum_t dy[t, n] x[t, k] (proqa_linear_wgrad_f16), and the cases
tests/test_wgrad_host.py and tests/test_wgrad_gpu.py share.

reference()      float64 on the kernel's own fp16 inputs.
restated_fp32()  "the reference's own arithmetic" under apex O1 with fp32 master gradients: an fp32 running sum over t in
                 ascending order, one product (exact: two 11-bit significands) and one add per term.
rel_err()        the project's max|a - ref| / max|ref| per tensor.
"""
import functools

import numpy as np
import torch

T_VALUES = (1, 7, 64, 65, 300, 1027, 4096)
SHAPES = ((128, 128), (384, 128), (512, 128), (128, 512), (200, 72), (768, 768))      # (200, 72): the edge-tile case


def _gaussian_cases():
    cases = [(T, N, K) for (N, K) in ((128, 128), (200, 72)) for T in T_VALUES]
    cases += [(T, N, K) for T in (300, 1027) for (N, K) in SHAPES if (T, N, K) not in cases]
    return tuple(cases)


GAUSSIAN_CASES = _gaussian_cases()      # 14 + 8: every T with (128, 128) and (200, 72), every shape with T = 300 and 1027
EXACT_CASES = tuple((T, N, K) for T in (65, 1027, 4096) for (N, K) in ((128, 128), (200, 72)))
BERT_BASE_SHAPES = ((2304, 768), (768, 768), (3072, 768), (768, 3072))
BERT_BASE_TOKENS = (81920, 8192)


def _seed(T, N, K):
    return (T * 1000003 + N * 1009 + K) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def gaussian_inputs(T, N, K):
    """seeded N(0, 1) fp16 (dy [T, N], x [T, K]), CPU"""
    gen = torch.Generator().manual_seed(_seed(T, N, K))
    return torch.randn((T, N), generator=gen).half(), torch.randn((T, K), generator=gen).half()


@functools.lru_cache(maxsize=None)
def integer_inputs(T, N, K):
    """seeded integer-valued fp16 in [-8, 8] (dy, x) and an integer-valued fp32 dw0 in [-1000, 1000], CPU.  Every partial
    sum of dw0 + sum_t dy x stays below 1000 + 64 * 4096 < 2^24: exact in fp32 in any order."""
    gen = torch.Generator().manual_seed(_seed(T, N, K) + 1)
    dy = torch.randint(-8, 9, (T, N), generator=gen).half()
    x = torch.randint(-8, 9, (T, K), generator=gen).half()
    dw0 = torch.randint(-1000, 1001, (N, K), generator=gen).float()
    return dy, x, dw0


def reference(dy, x, dw0=None):
    """float64 [N, K] of the fp16 inputs"""
    out = dy.double().t() @ x.double()
    return out if dw0 is None else out + dw0.double()


def restated_fp32(dy, x, dw0=None):
    """fp32 running sum over t ascending, one product and one add per term, vectorised over [N, K]"""
    a, b = dy.float().numpy(), x.float().numpy()
    acc = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32) if dw0 is None else dw0.float().numpy().copy()
    for t in range(a.shape[0]):
        acc += a[t][:, None] * b[t][None, :]
    return torch.from_numpy(acc)


def rel_err(got, ref):
    ref = ref.double()
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


@functools.lru_cache(maxsize=None)
def gaussian_reference(T, N, K):
    return reference(*gaussian_inputs(T, N, K))


def measure_reference_error(cases=GAUSSIAN_CASES):
    """{(T, N, K): rel_err(restated_fp32, reference)} over the Gaussian cases -- CPU only"""
    return {c: rel_err(restated_fp32(*gaussian_inputs(*c)), gaussian_reference(*c)) for c in cases}
