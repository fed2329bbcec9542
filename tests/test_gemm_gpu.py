"""proqa_gemm_tn_f16 (csrc/gemm_kernels.hip: 256 x 256 x 64 MFMA tiles, LDS-DMA ring, anti-phase K loop, persistent
workgroups on an XCD-aware tile walk, fitted GELU) against float64, element by element, under the bounds derived in
tests/gemm_oracle.py (GAMMA_gemm = 4 x the measured error of a float32 restatement; the GELU's documented fit error FIT;
tests/test_gemm_host.py reproduces the measurement and shows which kernel errors the bounds catch).  Every comparison covers
every output.  The shapes are the smallest that reach each path of the tile walk and each wrap of the two-deep ring; the
walk's model says which workgroup owns a failing element."""
import numpy as np
import pytest
import torch

import gemm_oracle as G

O = G.O
pytestmark = pytest.mark.gpu
SENTINEL = 7.0
EINVAL = -1
GUARD = 256                                           # sentinel rows in front of and behind Y


@pytest.fixture(scope="module")
def lib(gpu_device):
    from proqa_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def n_cus(gpu_device):
    return torch.cuda.get_device_properties(gpu_device).multi_processor_count


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def at_offset(t, elements):
    """A copy of t that starts `elements` fp16 values into its own allocation."""
    buf = torch.empty(t.numel() + elements, dtype=t.dtype, device=t.device)
    out = buf[elements:].view(t.shape)
    out.copy_(t)
    return out


class Output:
    """Y [M, N] in the middle of a larger allocation: GUARD sentinel rows (and `offset` elements) in front, GUARD rows behind;
    Y itself poisoned with NaN."""

    def __init__(self, M, N, device, offset=0):
        self.buf = torch.full(((M + 2 * GUARD) * N + offset,), SENTINEL, dtype=torch.float16, device=device)
        self.lo = offset + GUARD * N
        self.y = self.buf[self.lo:self.lo + M * N].view(M, N)
        self.y.fill_(float("nan"))

    def bits(self):
        """Y's bit patterns, after checking that nothing around Y was written."""
        assert bool((self.buf[:self.lo] == SENTINEL).all()), "written in front of Y"
        assert bool((self.buf[self.lo + self.y.numel():] == SENTINEL).all()), "written behind Y"
        return self.y.view(torch.int16)

    def host(self):
        return self.bits().cpu().numpy().view(np.float16)


def launch(lib, x, w, bias, y, epi):
    from proqa_amd import _lib
    (M, K), N = x.shape, w.shape[0]
    _lib.check(lib.proqa_gemm_tn_f16(x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(),
                                     M, N, K, epi, _lib.current_stream_ptr()))


def run(lib, device, x, w, bias, epi, offset=0):
    """x, w, bias: device tensors.  -> Output"""
    out = Output(x.shape[0], w.shape[0], device, offset)
    launch(lib, x, w, bias, out.y, epi)
    torch.cuda.synchronize()
    return out


def report(what, got, ref, epi, case, n_cus):
    """Print the worst |got - ref| / tol and assert that no output is outside the bound; a failure names the worst element, its
    tile, its place in the tile and the workgroup of the walk's model that owns it."""
    bad = ref.outside(got, epi)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ratio = np.abs(O.f64(got) - ref.out(epi)) / ref.bound(epi)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    finite = ratio[np.isfinite(ratio) & ~bad]
    print(f"{what}: worst |got - ref| / tol = {finite.max() if finite.size else 0:.3f}; {int(bad.sum())} of {bad.size} outside")
    if bad.any():
        worst = np.unravel_index(np.argmax(np.where(bad, ratio, -1.0)), bad.shape)
        tiles = sorted({(int(m) // G.TILE, int(n) // G.TILE) for m, n in zip(*np.nonzero(bad))})
        pytest.fail(f"{what}: {int(bad.sum())} outputs outside the bound in {len(tiles)} tiles {tiles[:12]}; worst "
                    f"{G.describe(worst, *case, n_cus)}: got {got[worst]}, reference {ref.out(epi)[worst]:.9g}, "
                    f"tolerance {ref.bound(epi)[worst]:.3g}")


def assert_exact(what, got, want, case, n_cus):
    bad = ~(O.f64(got) == want)
    print(f"{what}: {int(bad.sum())} of {bad.size} differ from float64")
    if bad.any():
        first = tuple(int(i[0]) for i in np.nonzero(bad))
        pytest.fail(f"{what}: {int(bad.sum())} outputs differ; first {G.describe(first, *case, n_cus)}: got {got[first]}, "
                    f"exact {want[first]}")


# ---- the walk's model on this device -----------------------------------------------------------------------------------
def test_the_case_list_reaches_every_path_on_this_device(n_cus):
    for case in G.CASES:
        assert (G.visits(*case, n_cus) == 1).all(), case
    reached = G.labels_reached(n_cus)
    missing = set(G.PATH_LABELS) - reached
    print(f"{n_cus} CUs; path labels reached: {sorted(reached)}" + (f"; NOT reached on this device: {sorted(missing)}" if missing else ""))
    assert missing <= {"grid_capped"}


# ---- bounds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("case", G.CASES, ids=["x".join(map(str, c)) for c in G.CASES])
def test_every_output_against_float64(lib, gpu_device, n_cus, case, family):
    x, w, bias = G.inputs(*case, family)
    ref = G.GemmRef(x, w, bias)
    tx, tw, tb = (dev(a, gpu_device) for a in (x, w, bias))
    for epi in (0, 1, 2):
        got = run(lib, gpu_device, tx, tw, tb, epi).host()
        what = f"gemm {case} {family} epilogue {epi}"
        if family == "int" and epi < 2:
            assert np.abs(ref.pre(epi)).max() <= 2048
            assert_exact(what, got, ref.pre(epi), case, n_cus)
        else:
            report(what, got, ref, epi, case, n_cus)
        if family == "overflow":
            pre = ref.pre(epi)
            assert (np.abs(pre) > 65520).any()
            if epi < 2:
                assert (O.f64(got)[np.abs(pre) > 65520] == np.copysign(np.inf, pre)[np.abs(pre) > 65520]).all()
            else:                                   # gelu(-huge) is 0, not -Inf
                assert (O.f64(got)[pre < -65520] == 0).all() and np.isposinf(O.f64(got)[pre > 65520]).all()


@pytest.mark.parametrize("zero_bias", [False, True], ids=["mixed", "bias0"])
def test_every_finite_fp16_through_the_epilogues(lib, gpu_device, n_cus, zero_bias):
    x, w, bias = G.every_fp16_inputs(zero_bias)
    ref = G.EveryFp16Ref(x, w, bias)
    tx, tw, tb = (dev(a, gpu_device) for a in (x, w, bias))
    case = G.EVERY_FP16_SHAPE
    got = run(lib, gpu_device, tx, tw, tb, 0).host()
    assert_exact("every fp16 value times 1 (subnormals included)", got, ref.x, case, n_cus)
    for epi in (1, 2):
        got = run(lib, gpu_device, tx, tw, tb, epi).host()
        report(f"every fp16 value + bias, epilogue {epi}", got, ref, epi, case, n_cus)
    steps = G.ulps_off(got, ref.out(2))
    print(f"fitted GELU: {100 * (steps > 0).mean():.2f} % of {steps.size} outputs are one fp16 step from the correctly rounded "
          f"result (the float32 restatement: 2.2 %); largest distance {int(steps.max())} steps")
    assert steps.max() <= 1


# ---- borders -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES, ids=["x".join(map(str, c)) for c in G.CASES])
def test_nothing_outside_y_is_written_and_16_byte_offsets_change_nothing(lib, gpu_device, case):
    """Y between sentinel rows; then X, W, bias and Y each 8 elements (16 bytes) into their allocations: the same bits."""
    x, w, bias = (dev(a, gpu_device) for a in G.inputs(*case, "gauss"))
    xo, wo, bo = (at_offset(t, 8) for t in (x, w, bias))
    assert all(t.data_ptr() % 256 == 0 for t in (x, w, bias)) and all(t.data_ptr() % 256 == 16 for t in (xo, wo, bo))
    for epi in (0, 2):
        aligned = run(lib, gpu_device, x, w, bias, epi)
        shifted = run(lib, gpu_device, xo, wo, bo, epi, offset=8)
        assert aligned.y.data_ptr() % 16 == 0 and shifted.y.data_ptr() % 256 == (aligned.y.data_ptr() + 16) % 256
        a, s = aligned.bits(), shifted.bits()
        assert not bool(torch.isnan(aligned.y).any()), "a part of Y was not written"
        assert torch.equal(a, s), (case, epi)


# ---- confinement ---------------------------------------------------------------------------------------------------------
def test_a_non_finite_operand_stays_in_its_row_and_column(lib, gpu_device):
    """One +Inf in X[m0, k0] reaches row m0 only, one NaN in W[n0, k0] column n0 only: the last slab, the last group of
    feature tiles, the last K-step -- what a ring or a tile walk that mixes rows would spread."""
    M, N, K = case = (2304, 2304, 192)
    m0, n0, k0 = M - 5, N - 3, K - 3
    x, w, bias = (dev(a, gpu_device) for a in G.inputs(*case, "gauss"))
    x_inf, w_nan = x.clone(), w.clone()
    x_inf[m0, k0] = float("inf")
    w_nan[n0, k0] = float("nan")
    other_rows = torch.arange(M, device=gpu_device) != m0
    other_cols = torch.arange(N, device=gpu_device) != n0
    for epi in (1, 2):
        clean = run(lib, gpu_device, x, w, bias, epi)
        assert bool(torch.isfinite(clean.y).all())
        got = run(lib, gpu_device, x_inf, w, bias, epi)
        assert torch.equal(got.bits()[other_rows], clean.bits()[other_rows]), epi
        hit = ~torch.isfinite(got.y[m0])
        print(f"epilogue {epi}: +Inf in X[{m0}, {k0}] makes {int(hit.sum())} of {N} outputs of row {m0} non-finite")
        if epi == 1:                                # (the GELU maps -Inf to 0: only the plain epilogues show every product)
            assert bool(hit[w[:, k0] != 0].all())
        got = run(lib, gpu_device, x, w_nan, bias, epi)
        assert torch.equal(got.bits()[:, other_cols], clean.bits()[:, other_cols]), epi
        hit = torch.isnan(got.y[:, n0])
        print(f"epilogue {epi}: NaN in W[{n0}, {k0}] makes {int(hit.sum())} of {M} outputs of column {n0} NaN")
        if epi == 1:
            assert bool(hit.all())


# ---- repeatability ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES, ids=["x".join(map(str, c)) for c in G.CASES])
def test_a_launch_repeats_bit_for_bit_also_after_another_shape(lib, gpu_device, case):
    """Twice into NaN-poisoned outputs, then once more after a launch of another shape (another ring history, another number
    of barriers): three launches of the case, the same bits.  The race screen under load is test_encoder_gpu.py's."""
    x, w, bias = (dev(a, gpu_device) for a in G.inputs(*case, "gauss"))
    other = (512, 256, 64) if case[2] != 64 else (256, 512, 192)
    ox, ow, ob = (dev(a, gpu_device) for a in G.inputs(*other, "gauss"))
    first = run(lib, gpu_device, x, w, bias, 2)
    second = run(lib, gpu_device, x, w, bias, 2)
    run(lib, gpu_device, ox, ow, ob, 0).bits()
    third = run(lib, gpu_device, x, w, bias, 2)
    assert not bool(torch.isnan(first.y).any())
    assert torch.equal(first.bits(), second.bits()) and torch.equal(first.bits(), third.bits())


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_what_the_entry_point_refuses_is_never_launched(lib, gpu_device):
    M, N, K = 256, 256, 64
    x = torch.ones((M, K), dtype=torch.float16, device=gpu_device)
    w = torch.ones((N, K), dtype=torch.float16, device=gpu_device)
    b = torch.ones(N, dtype=torch.float16, device=gpu_device)
    out = Output(M, N, gpu_device)
    out.y.fill_(SENTINEL)
    X, W, B, Y = x.data_ptr(), w.data_ptr(), b.data_ptr(), out.y.data_ptr()
    assert all(p % 16 == 0 for p in (X, W, B, Y))
    stream = torch.cuda.current_stream().cuda_stream

    def refused(xp, wp, bp, yp, m, n, k, epi, names=None):
        assert lib.proqa_gemm_tn_f16(xp, wp, bp, yp, m, n, k, epi, stream) == EINVAL, (m, n, k, epi)
        if names is not None:
            assert f"{names} is not 16-byte aligned" in lib.proqa_last_error().decode()

    for m, n, k in [(255, N, K), (257, N, K), (M, 255, K), (M, 128, K), (M, 0, K), (M, N, 63), (M, N, 32), (M, N, 96), (M, N, 0),
                    (-256, N, K)]:
        refused(X, W, B, Y, m, n, k, 0)
    for epi in (3, -1):
        refused(X, W, B, Y, M, N, K, epi)
    for epi in (1, 2):
        refused(X, W, None, Y, M, N, K, epi)
    refused(None, W, B, Y, M, N, K, 0)
    refused(X, None, B, Y, M, N, K, 0)
    refused(X, W, B, None, M, N, K, 0)
    for step in (2, 8):                             # a pointer that is not 16-byte aligned is refused by name, never launched
        refused(X + step, W, B, Y, M, N, K, 2, "x")
        refused(X, W + step, B, Y, M, N, K, 2, "w")
        refused(X, W, B + step, Y, M, N, K, 2, "bias")
        refused(X, W, B + step, Y, M, N, K, 0, "bias")
        refused(X, W, B, Y + step, M, N, K, 2, "y")
        refused(X, W, B, Y + step, 0, N, K, 2, "y")
    assert lib.proqa_gemm_tn_f16(X, W, B, Y, 0, N, K, 2, stream) == 0          # no rows: fine, and nothing is written
    assert lib.proqa_gemm_tn_f16(X, W, None, Y, 0, N, K, 0, stream) == 0
    torch.cuda.synchronize()
    assert bool((out.bits() == torch.tensor(SENTINEL, dtype=torch.float16).view(torch.int16).item()).all())
    launch(lib, x, w, None, out.y, 0)                # and the accepted call with the same arguments does write: 64 ones
    torch.cuda.synchronize()
    assert bool((out.y == 64).all()) and out.bits() is not None
