"""Float64 reference, derived bounds, the shared case list and a model of the tile walk for the hand-written dense layer
proqa_gemm_tn_f16 (csrc/gemm_kernels.hip):  Y[M, N] = epilogue(X[M, K] . W[N, K]^T + bias[N]),  epilogue 0 none, 1 + bias,
2 erf-GELU(. + bias).  NumPy / torch-CPU only: tests/test_gemm_host.py runs it without a GPU, tests/test_gemm_gpu.py holds
the kernel to it.  The references, ulp16, final_rounding and the GELU pieces are those of tests/encoder_ops_oracle.py.

BOUNDS.  The reference is float64 x w^T (+ bias), then gelu_ref, on the kernel's own fp16 operands, compared element by
element under the project's rule (header of encoder_ops_oracle.py):

    t = GAMMA_gemm x 2^-24 (sum_k |x_k| |w_k| + |bias|)                                   the fp32 sum
    epilogues 0, 1:   tol = final_rounding(ref, t) + t
    epilogue 2:       e = 1.13 t + FIT a Phi(-a) + GAMMA_gelu gelu_unit(pre),  a = min(|pre|, 6);  tol = final_rounding(ref, e) + e

Where the correctly rounded result is not finite (beyond fp16's range) the output must be that infinity.

FIT = 4.6e-5 is NOT a fitted slack: it is the approximation the kernel documents for its own GELU (gelu_erf4: Phi(-a) =
2^q(a) with a degree-6 fit of log2 Phi(-a) on [0, 6], |error| <= 6.5e-5 in the exponent = 4.6e-5 relative to Phi(-a);
gelu(x) = max(x, 0) - a Phi(-a), so the error of the result is at most FIT a Phi(-a)).  GAMMA_gelu is the existing
GAMMA["gelu"].  GAMMA_gemm is MEASURED, never fitted to the kernel: measure_reference_error() evaluates the float32
restatement below (f32(x) @ f32(w).T in the BLAS' order, the bias added in float32) against float64 on this file's own case
list and families, takes the largest |f32 - f64| / (2^-24 (sum |x| |w| + |bias|)), and GAMMA_gemm = 4 x that (the factor 4:
what the restatement does not share with the kernel -- the MFMA accumulation order, v_exp_f32 a couple of ulps off).  It
also reports what gelu_erf4_f32 (the kernel's GELU restated operation by operation with its coefficients, one rounding per
fma) needs of GAMMA_gelu once FIT is granted.  A kernel that misses a bound is a finding to explain, not a constant to raise.

MEASURED (python tests/gemm_oracle.py prints the table; tests/test_gemm_host.py reproduces it):

    gemm         2^-24 (sum_k |x_k| |w_k| + |bias|)                      %(gemm)s
    gelu_erf4    2^-24 |t| (1 + |t|), after 1.13 t_err + FIT a Phi(-a)   %(gelu_erf4)s    (reported; the bound uses GAMMA["gelu"] = %(gamma_gelu).3f)
"""
import math

import numpy as np
import torch

import encoder_ops_oracle as O
from encoder_ops_oracle import DenseRef, final_rounding, gelu_ref, gelu_unit, h16, rng_of, f32, f64, U24

# measure_reference_error() on the CPU: worst ratio over CASES x the inexact families
REFERENCE_RATIO = {
    "gemm": 6.5890,           # GAMMA = 26.356
    "gelu_erf4": 0.2105,      # (GAMMA["gelu"] = 4.4512 is the one the bound uses)
}
GAMMA_GEMM = 4.0 * REFERENCE_RATIO["gemm"]
GAMMA_GELU = O.GAMMA["gelu"]
FIT = 4.6e-5
__doc__ = __doc__ % {"gemm": f"worst ratio {REFERENCE_RATIO['gemm']:.3f}    GAMMA = 4 x = {GAMMA_GEMM:.3f}",
                     "gelu_erf4": f"worst ratio {REFERENCE_RATIO['gelu_erf4']:.3f}", "gamma_gelu": GAMMA_GELU}

TILE, BK, GROUP = 256, 64, 8

# The smallest shapes that reach each path of the tile walk on 256 CUs (schedule_model / path_labels below say which)
CASES = (
    (256, 256, 64), (256, 256, 128), (256, 256, 192), (256, 256, 256),     # one tile; 1, 2, 3, 4 K-steps
    (256, 512, 64), (256, 768, 192),          # one workgroup walks several tiles; XCDs without a slab
    (512, 256, 128),                          # two workgroups, one tile each
    (768, 512, 320),                          # five K-steps
    (2304, 256, 64),                          # two slabs on XCD 0, one feature tile
    (2304, 2304, 64), (2304, 2304, 192),      # 9 x 9 tiles: two groups (ragged last group of 1), two slabs on XCD 0,
    #                                           workgroups of several, one and no tiles
    (2560, 2816, 128),                        # the same with a ragged last group of 3
    (8448, 2048, 64),                         # 264 tiles: the grid is capped at the CU count
    (1024, 768, 3072),                        # 48 K-steps
)
FAMILIES = ("gauss", "int", "subnormal", "overflow")
EVERY_FP16_SHAPE = (1024, 256, 64)
CU_COUNTS = (8, 13, 32, 64, 256, 304)


# ------------------------------------------------------------------------------------------------------------------
# The tile walk (the slot arithmetic at the head of gemm_tn_f16 and its tile_bases) and the entry point's grid
# ------------------------------------------------------------------------------------------------------------------
def grid_size(M, N, n_cus, floor=True):
    tiles = (M // TILE) * (N // TILE)
    return min(tiles, max(n_cus, 8) if floor else n_cus)


def schedule_model(M, N, K, n_cus, floor=True):
    """The (token slab, feature tile) sequence of every workgroup, in launch order of the workgroups.  floor: the entry
    point launches at least 8 workgroups wherever there are 8 tiles; without it a device of fewer than 8 CUs leaves the slabs
    of the missing residues of blockIdx.x & 7 uncomputed."""
    tiles_n, tiles_m = N // TILE, M // TILE
    grid = grid_size(M, N, n_cus, floor)
    walk = []
    for b in range(grid):
        xcd, slot, n_slots = b & 7, b >> 3, (grid + 7 - (b & 7)) >> 3
        my_slabs = (tiles_m - xcd + 7) >> 3
        my_tiles = my_slabs * tiles_n
        seq = []
        for t in range(slot, my_tiles, n_slots):
            per_full_group = my_slabs * GROUP
            grp = t // per_full_group
            g = min(tiles_n - grp * GROUP, GROUP)
            r = t - grp * per_full_group
            seq.append((xcd + 8 * (r // g), grp * GROUP + r % g))
        walk.append(seq)
    return walk


def visits(M, N, K, n_cus, floor=True):
    """[tiles_m, tiles_n] count of the workgroups that compute each tile."""
    count = np.zeros((M // TILE, N // TILE), np.int64)
    for seq in schedule_model(M, N, K, n_cus, floor):
        for slab, nt in seq:
            count[slab, nt] += 1
    return count


def owner(M, N, K, n_cus, slab, nt):
    """(workgroup, position in its sequence) of the tile."""
    for b, seq in enumerate(schedule_model(M, N, K, n_cus)):
        if (slab, nt) in seq:
            return b, seq.index((slab, nt))
    return None, None


PATH_LABELS = ("one_tile_workgroup", "several_tile_workgroup", "xcd_without_slab", "idle_workgroup", "two_slabs_per_xcd",
               "several_groups", "ragged_group_of_1", "ragged_group_of_3", "two_slabs_and_ragged_group", "grid_capped",
               "k_steps_1", "k_steps_2", "k_steps_3", "k_steps_4", "k_steps_5", "k_steps_48")


def path_labels(M, N, K, n_cus):
    walk = schedule_model(M, N, K, n_cus)
    tiles_m, tiles_n = M // TILE, N // TILE
    labels = {f"k_steps_{K // BK}"} & set(PATH_LABELS)
    if any(len(s) == 1 for s in walk):
        labels.add("one_tile_workgroup")
    if any(len(s) > 1 for s in walk):
        labels.add("several_tile_workgroup")
    if any(not s for s in walk):
        labels.add("idle_workgroup")
    if tiles_m < min(len(walk), 8):
        labels.add("xcd_without_slab")
    if tiles_m > 8:
        labels.add("two_slabs_per_xcd")
    if tiles_n > GROUP:
        labels.add("several_groups")
        if tiles_n % GROUP in (1, 3):
            labels.add(f"ragged_group_of_{tiles_n % GROUP}")
        if tiles_n % GROUP and tiles_m > 8:
            labels.add("two_slabs_and_ragged_group")
    if tiles_m * tiles_n > n_cus:
        labels.add("grid_capped")
    return labels


def labels_reached(n_cus, cases=CASES):
    out = set()
    for M, N, K in cases:
        out |= path_labels(M, N, K, n_cus)
    return out


def describe(index, M, N, K, n_cus):
    """Where an output element lies: tile, position in the tile, and the workgroup of the model that computes it."""
    m, n = (int(i) for i in index)
    b, pos = owner(M, N, K, n_cus, m // TILE, n // TILE)
    return (f"Y[{m}, {n}]: tile (slab {m // TILE}, feature tile {n // TILE}), row {m % TILE} / feature {n % TILE} of the tile, "
            f"tile {pos} of workgroup {b} ({n_cus} CUs)")


# ------------------------------------------------------------------------------------------------------------------
# Inputs
# ------------------------------------------------------------------------------------------------------------------
def feature_pattern(N):
    """Integers in [-4, 4] that differ between feature n and n + 1, n + 8 (but for the 8 features in front of a tile edge)
    and n + 256."""
    n = np.arange(N)
    return ((n + n // TILE) % 9 - 4).astype(np.float64)


def inputs(M, N, K, family):
    """(x [M, K], w [N, K], bias [N]) as fp16.
    gauss      N(0, 1) x N(0, 1 / K), bias 0.5 N(0, 1)
    int        small integers in the style of dense_inputs(kind="int"): every fp32 partial sum is exact and |y| <= 2048,
               so epilogues 0 and 1 equal float64 bit for bit; the bias differs from feature to feature
    subnormal  x = +-j 2^-24, j in [1, 1023] (fp16's subnormals), w = 2^10 N(0, 1): the outputs are normal numbers
    overflow   the int family with the weight and the bias times 1024: still exact in fp32 (integers x 2^10 below 2^24),
               |pre| of the order of 3e4, so a few per cent pass +-65504 -- exactly, not within a rounding of the edge"""
    r = rng_of("gemm", M, N, K, family)
    if family == "gauss":
        x, w, bias = r.standard_normal((M, K)), r.standard_normal((N, K)) / math.sqrt(K), 0.5 * r.standard_normal(N)
    elif family in ("int", "overflow"):
        x = r.integers(-3, 4, (M, K)).astype(np.float64)
        w = (r.integers(-3, 4, (N, K)) * (r.random((N, K)) < 64.0 / K)).astype(np.float64)
        bias = feature_pattern(N)
        if family == "overflow":
            w, bias = 1024.0 * w, 1024.0 * bias
    elif family == "subnormal":
        x = r.integers(1, 1024, (M, K)) * r.choice([-1.0, 1.0], (M, K)) * 2.0 ** -24
        w, bias = 1024.0 * r.standard_normal((N, K)), 0.25 * r.standard_normal(N)
    else:
        raise ValueError(family)
    return h16(x), h16(w), h16(bias)


def every_fp16_inputs(zero_bias=False):
    """Shape (1024, 256, 64).  X holds all 63 488 finite fp16 bit patterns (then zeros), W[n, k] = (k == n % 64), so
    Y[m, n] = epilogue(X[m, n % 64] + bias[n]); the bias gives every X value four different partners."""
    M, N, K = EVERY_FP16_SHAPE
    x = np.zeros(M * K, np.float16)
    x[:63488] = O.gelu_x_all_finite().reshape(-1)
    n = np.arange(N)
    w = (np.arange(K)[None, :] == (n % K)[:, None]).astype(np.float16)
    bias = np.array(O.GELU_BIAS_VALUES)[(n % 16 + 4 * (n // 64)) % 16]
    if zero_bias:
        bias = np.zeros(N)
    return x.reshape(M, K), w, h16(bias)


# ------------------------------------------------------------------------------------------------------------------
# Reference and bound
# ------------------------------------------------------------------------------------------------------------------
def phi_minus(a):
    """Phi(-a) in float64."""
    return (0.5 * torch.special.erfc(torch.from_numpy(f64(a)) / math.sqrt(2.0))).numpy()


def gelu_fit_bound(pre, t):
    """Epilogue 2's bound around gelu_ref(pre) for a pre-activation known to within t."""
    a = np.minimum(np.abs(pre), 6.0)
    e = 1.13 * t + FIT * a * phi_minus(a) + GAMMA_GELU * gelu_unit(pre)
    return final_rounding(gelu_ref(pre), e) + e


def outside(got, ref, tol):
    """Boolean map of the outputs outside the bound (a NaN is outside); where the correctly rounded reference is not finite
    the output must be that infinity."""
    with np.errstate(over="ignore"):
        expect = f64(h16(ref))
    got = f64(got)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(expect), ~(np.abs(got - ref) <= tol), got != expect)


class GemmRef:
    """The float64 product (one DenseRef, shared by the three epilogues) and the bound of each epilogue."""

    def __init__(self, x, w, bias):
        self.plain = DenseRef(x, w)
        self.bias = f64(bias)
        self._kept = {}

    def _keep(self, key, make):
        if key not in self._kept:
            self._kept[key] = make()
        return self._kept[key]

    def pre(self, epi):
        return self.plain.pre if epi == 0 else self.plain.pre + self.bias

    def mag(self, epi):
        return self.plain.mag if epi == 0 else self.plain.mag + np.abs(self.bias)

    def unit(self, epi):
        return U24 * self.mag(epi)

    def out(self, epi):
        return self._keep("out", lambda: gelu_ref(self.pre(2))) if epi == 2 else self.pre(epi)

    def bound(self, epi):
        def make():
            t = GAMMA_GEMM * self.unit(epi)
            if epi == 2:
                return gelu_fit_bound(self.pre(epi), t)
            return final_rounding(self.pre(epi), t) + t
        return self._keep("bound", make) if epi == 2 else make()     # (only the GELU's is costly enough to keep)

    def outside(self, got, epi):
        return outside(got, self.out(epi), self.bound(epi))


class EveryFp16Ref:
    """every_fp16_inputs: the sum has one non-zero term, so the pre-activation is x + bias rounded once to fp32."""

    def __init__(self, x, w, bias):
        cols = np.arange(w.shape[0]) % x.shape[1]
        self.x = f64(x)[:, cols]
        self.sum = self.x + f64(bias)

    def out(self, epi):
        return (self.x, self.sum, gelu_ref(self.sum))[epi]

    def bound(self, epi):
        t = U24 * np.abs(self.sum)
        if epi == 2:
            return gelu_fit_bound(self.sum, t)
        return final_rounding(self.sum, t) + t

    def outside(self, got, epi):
        if epi == 0:                                    # X's values exactly, subnormals included (+-0 compare as values)
            return f64(got) != self.x
        return outside(got, self.out(epi), self.bound(epi))


def ordinal16(a):
    """fp16 values on the integer line of their bit patterns (+-0 at 0, the infinities one step beyond +-65504)."""
    b = np.ascontiguousarray(h16(a)).view(np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def ulps_off(got, ref):
    """Distance in fp16 steps between the output and the correctly rounded reference."""
    with np.errstate(over="ignore"):
        return np.abs(ordinal16(got) - ordinal16(h16(ref)))


# ------------------------------------------------------------------------------------------------------------------
# float32 restatement of the kernel, and the mutants the bounds are meant to catch
# ------------------------------------------------------------------------------------------------------------------
GELU_COEFFS = (2.299005791428499e-05, 0.000611100229434669, 0.007195569109171629, 0.05118535831570625,
               -0.46127188205718994, 1.1501742601394653, -1.000064730644226)       # q in an = -a, as gelu_erf4 holds them
GELU_MUTANTS = ("tanh", "clamp4", "fit_doubled")


def fma32(a, b, c):
    """fma of float32 operands: the product is exact in float64; the sum is rounded to float64 and then to float32 (a double
    rounding differs from the single one for about one operand set in 2^29)."""
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)


def gelu_erf4_f32(x, mutant=None):
    """gelu_erf4 operation by operation on a float32 argument.  Mutants: 'tanh' (the tanh form), 'clamp4' (a clamped at 4),
    'fit_doubled' (the constant term of q a further 6.5e-5 off: twice the documented error in the exponent)."""
    x = f32(x)
    if mutant == "tanh":
        return O.gelu_f32(x, mutant="tanh")
    an = np.maximum(-np.abs(x), np.float32(-4.0 if mutant == "clamp4" else -6.0))
    c = [np.float32(v) for v in GELU_COEFFS]
    if mutant == "fit_doubled":
        c[6] = np.float32(GELU_COEFFS[6] - 6.5e-5)
    q = fma32(c[0], an, c[1])
    for k in range(2, 7):
        q = fma32(q, an, c[k])
    u = np.exp2(q, dtype=np.float32)
    return fma32(an, u, np.maximum(x, np.float32(0)))


GEMM_MUTANTS = ("skip_last_k_step", "stale_ring_buffer", "swapped_pieces", "neighbour_tile_bias", "bias_shifted_8",
                "slabs_exchanged", "last_tile_unwritten", "gelu_before_bias")


def gemm_f32(x, w, bias, epi, mutant=None, gelu_mutant=None, n_cus=256):
    """float32 restatement before the output rounding: f32(x) @ f32(w).T, the bias added in float32, gelu_erf4_f32.
    Mutants (what a wrong tile walk, ring or epilogue would do):
      skip_last_k_step     the last 64 of K are never accumulated
      stale_ring_buffer    the last K-step reads the ring buffer's previous content, the K-step two before it (K >= 192)
      swapped_pieces       16-byte pieces 2 and 5 (8 features each) of the last 64-feature block of the last tile change places
      neighbour_tile_bias  every feature tile adds the bias of the next one (cyclically)
      bias_shifted_8       feature n adds bias[n + 8] (cyclically)
      slabs_exchanged      the first and the last token slab change places
      last_tile_unwritten  the last tile of the longest sequence of schedule_model(.., n_cus) stays NaN
      gelu_before_bias     epilogue 2 as gelu(x w^T) + bias"""
    M, K = x.shape
    N = w.shape[0]
    x32, w32 = f32(x), f32(w)
    if mutant == "skip_last_k_step":
        x32, w32 = x32[:, :K - BK], w32[:, :K - BK]
    elif mutant == "stale_ring_buffer" and K >= 3 * BK:
        x32, w32 = x32.copy(), w32.copy()
        x32[:, K - BK:], w32[:, K - BK:] = x32[:, K - 3 * BK:K - 2 * BK], w32[:, K - 3 * BK:K - 2 * BK]
    y = x32 @ w32.T
    b32 = f32(bias)
    if mutant == "neighbour_tile_bias":
        b32 = np.roll(b32, -TILE)
    elif mutant == "bias_shifted_8":
        b32 = np.roll(b32, -8)
    if epi == 2 and mutant == "gelu_before_bias":
        y = gelu_erf4_f32(y, gelu_mutant) + b32
    else:
        if epi != 0:
            y = y + b32
        if epi == 2:
            y = gelu_erf4_f32(y, gelu_mutant)
    if mutant == "swapped_pieces":
        y = y.copy()
        a, b = y[M - TILE:, N - 64 + 16:N - 64 + 24].copy(), y[M - TILE:, N - 64 + 40:N - 64 + 48].copy()
        y[M - TILE:, N - 64 + 16:N - 64 + 24], y[M - TILE:, N - 64 + 40:N - 64 + 48] = b, a
    elif mutant == "slabs_exchanged" and M > TILE:
        y = y.copy()
        a = y[:TILE].copy()
        y[:TILE], y[M - TILE:] = y[M - TILE:], a
    elif mutant == "last_tile_unwritten":
        slab, nt = max(schedule_model(M, N, K, n_cus), key=len)[-1]
        y = y.copy()
        y[slab * TILE:(slab + 1) * TILE, nt * TILE:(nt + 1) * TILE] = np.nan
    return y


# ------------------------------------------------------------------------------------------------------------------
# The measurement behind GAMMA_gemm
# ------------------------------------------------------------------------------------------------------------------
def measure_reference_error(verbose=False, cases=CASES):
    """Worst |float32 restatement - float64| / unit over the case list and the families (the exact families measure 0).
    'gemm': the pre-activation with and without bias.  'gelu_erf4': what the restated GELU is off by beyond
    1.13 |pre32 - pre64| + FIT a Phi(-a), in GELU units, on the pre-activations of the list and on every finite fp16."""
    worst = {"gemm": 0.0, "gelu_erf4": 0.0}

    def note(op, case, r):
        worst[op] = max(worst[op], r)
        if verbose:
            print(f"  {op:10s} {str(case):44s} {r:8.3f}")

    def gelu_excess(pre32, pre64):
        a = np.minimum(np.abs(pre64), 6.0)
        diff = np.abs(f64(gelu_erf4_f32(pre32)) - gelu_ref(pre64)) - 1.13 * np.abs(f64(pre32) - pre64) - FIT * a * phi_minus(a)
        return np.maximum(diff, 0.0)

    for M, N, K in cases:
        for family in FAMILIES:
            x, w, bias = inputs(M, N, K, family)
            ref = GemmRef(x, w, bias)
            for epi in (0, 1):
                pre32 = gemm_f32(x, w, bias, epi)
                note("gemm", (M, N, K, family, epi), O._ratio(pre32 - ref.pre(epi), ref.unit(epi)))
            if family in ("gauss", "subnormal"):
                note("gelu_erf4", (M, N, K, family), O._ratio(gelu_excess(pre32, ref.pre(1)), gelu_unit(ref.pre(1))))
    for zero_bias in (False, True):
        x, w, bias = every_fp16_inputs(zero_bias)
        ref = EveryFp16Ref(x, w, bias)
        with np.errstate(over="ignore"):
            pre32 = gemm_f32(x, w, bias, 1)
            fin = np.isfinite(h16(ref.out(2)))
            note("gelu_erf4", ("every_fp16", zero_bias), O._ratio(gelu_excess(pre32, ref.sum)[fin], gelu_unit(ref.sum)[fin]))
    return worst


if __name__ == "__main__":
    m = measure_reference_error(verbose=True)
    for op, r in m.items():
        print(f'    "{op}": {r:.4f},      # x 4 = {4 * r:.4f}')
    print("path labels at 256 CUs:", sorted(labels_reached(256)))
