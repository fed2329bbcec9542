"""kmeans_assign (csrc/kmeans_kernels.hip) against oracle/kmeans_oracle.py in float64, on the kernel's own fp16 points and
fp32 centroids, at the sizes, scales and near-ties where the kernel changes path.

THE RULE (check_against_float64, used by every case).  With s64(i, c) = x_i.c - |c|^2/2 (L2) or x_i.c (IP) in float64:

  labels     s64(i, got_i) >= s64(i, best_i) - tol_i for every point; no label outside [0, k); where two centroid rows are
             bit-identical the higher index never appears.
  distances  |D_i - d64(i, got_i)| <= 2 tol_i + 2^-24 (|x_i|^2 + |c_got|^2)   (L2; d64 clipped at 0 like the oracle's)
             |D_i - s64(i, got_i)| <= 2 tol_i + 2^-24 |s64(i, got_i)|         (IP)

  tol_i = representation term + accumulation term.
  representation  |x_i| max_c |c - (hi + lo)| + max_c |h_c - stored terms|, computed exactly from the documented operand
                  format (operand_format below: hi + lo fp16 split of every component; for L2 the norm term
                  h = -|c_seen|^2/2 as the five fp16 terms a, b, cc, p, p2 of prep_centroids).  It is the format's error,
                  not the kernel's; below 2^-3 the lo parts are fp16 subnormals, so it matters for small-scale data.
  accumulation    GAMMA (|x_i| max|c| + max|c|^2/2)   (IP: GAMMA |x_i| max|c|, there is no norm term to add).
                  GAMMA is measured, not chosen: the largest deviation, in these units, of a plain float32 NumPy
                  evaluation of the same scores from float64 over every case of this file (measure_reference_error(), CPU
                  only), times 4 -- the factor this project gives device summation order over the host's
                  (tests/test_inbatch_gpu.py, K_INTRINSICS).

      measured float32 deviation   6.148e-07 (scale-1-ip), recorded rounded up: REFERENCE_DEVIATION = 6.2e-07
      GAMMA = 4 x that             2.48e-06
      the nominating pass assumes  4e-5 for its own summation (kmeans_kernels.hip, margin[]): GAMMA is 16 times below it

Every case not built as a near-tie case must leave at most 1 % of its points with a float64 lead below tol_i (asserted on
the CPU before the GPU call), so the label rule amounts to equality with the oracle almost everywhere; the table at the end
of this header has the share of every case.

THE ROUTES (run_routes).  Every case goes through
  two-pass   MODE_NOMINATE + MODE_SELECTED, the default;
  hinted     the same on a handle that has run proqa_kmeans_update_device on the same points (the nominating pass then
             walks them in that update's sorted order), hinted with the right labels, random ones and out-of-range ones;
  full       MODE_FULL, which a handle created with n_max < n takes (n = 1: the point is sent twice, n_max = 1);
each must pass the rule and all must return identical labels.

MEASURED (measure_reference_error(), `python tests/test_kmeans_assign_gpu.py` prints every case; deviation of the float32
evaluation in units of the accumulation term, share = points whose float64 lead is below tol_i; cases not named: 0.00 %):

    family    metric  cases   deviation    share
    k         l2      12      <= 3.83e-07  0.00 %
    k         ip      12      <= 5.68e-07  0.00 %
    bigk      l2       2      <= 3.42e-07  0.00 %
    n         l2      11      <= 4.36e-07  0.00 %
    n         ip      11      <= 5.65e-07  0.00 %
    negative  l2       2      <= 1.02e-07  0.00 %
    negative  ip       2      <= 4.87e-07  0.00 %
    scale     l2       4      <= 3.99e-07  0.00 %
    scale     ip       4      <= 6.15e-07  0.00 %
    old       l2       3      <= 1.18e-07  3000x37: 0.03 %, 20000x300: 0.03 %
    old       ip       3      <= 1.96e-07  20000x300: 0.01 %
    norm      l2       4      <= 3.76e-07  0.00 %   (|c| = 409, 523, 5000, 50000)
    integers  l2       1         2.01e-07  0.05 %
    twins     l2       2      <= 3.89e-07  78.60 % (scale 1), 80.45 % (scale 0.05)   near-tie cases: the 1 % condition
    twins     ip       2      <= 5.76e-07   2.40 % (scale 1),  3.95 % (scale 0.05)   does not apply
    (twins, L2, on the CPU: the hi-only argmax differs from the float64 one for 48 % / 47 % of the points, and 35 % / 43 % of
    them have a float64 lead below 2^-20 |x| max|c|)

On the device (MI355X, this file's first run): the worst label deficit is 0.11 tol (twins, scale 0.05, L2; 107 labels differ
from the oracle's there, 58 at scale 1, none in any other case), the worst distance error 0.92 of its allowance (scale 1e-3,
L2: twice the norm term's representation error, which fp16 subnormals set -- the format's error, reached exactly).
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import kmeans_oracle

gpu = pytest.mark.gpu

REFERENCE_DEVIATION = 6.2e-07
GAMMA = 4.0 * REFERENCE_DEVIATION
NOMINATION_ALLOWANCE = 4e-5             # kmeans_kernels.hip, margin[]
MAX_NEAR_TIE_SHARE = 0.01
NORM_SCALE = 32768.0                    # kNormScale
D = 128


# ---- the operand format, restated on the CPU ---------------------------------------------------------------------------------

def _f16(v):
    return np.asarray(v, np.float32).astype(np.float16)


def operand_format(c, l2):
    """(hi, lo, h_stored): what prep_centroids lays out for fp32 centroids c -- the fp16 parts of every component and, for L2,
    the float64 sum of the five fp16 norm terms (fine a, b, cc against 1; coarse p, p2 against 2^15).  The norm is the fp32
    tree sum of the squares of hi + lo in the kernel's order."""
    c = np.asarray(c, np.float32)
    hi = c.astype(np.float16)
    lo = (c - hi.astype(np.float32)).astype(np.float16)
    if not l2:
        return hi, lo, np.zeros(len(c))
    seen = hi.astype(np.float32) + lo.astype(np.float32)
    red = (seen * seen).astype(np.float32)
    s = 64
    while s > 0:
        red[:, :s] = red[:, :s] + red[:, s:2 * s]
        s >>= 1
    h = (np.float32(-0.5) * red[:, 0]).astype(np.float32)
    big = np.abs(h) >= NORM_SCALE
    p = np.where(big, _f16(h / np.float32(NORM_SCALE)), np.float16(0))
    h1 = (h - p.astype(np.float32) * np.float32(NORM_SCALE)).astype(np.float32)
    p2 = np.where(big, _f16(h1 / np.float32(NORM_SCALE)), np.float16(0))
    h2 = (h1 - p2.astype(np.float32) * np.float32(NORM_SCALE)).astype(np.float32)
    a = _f16(h2)
    b = _f16(h2 - a.astype(np.float32))
    cc = _f16((h2 - a.astype(np.float32)).astype(np.float32) - b.astype(np.float32))
    stored = (p.astype(np.float64) + p2.astype(np.float64)) * NORM_SCALE + a.astype(np.float64) + b.astype(np.float64) \
        + cc.astype(np.float64)
    return hi, lo, stored


# ---- cases: (x fp16 [n, 128], c fp32 [k, 128], l2, near_tie) ------------------------------------------------------------------

def _seed(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key))


def clustered(rng, n, k, scale, spread=0.3):
    c = (scale * rng.standard_normal((k, D))).astype(np.float32)
    x = (c[rng.integers(0, k, n)] + spread * scale * rng.standard_normal((n, D))).astype(np.float16)
    return x, c


@functools.lru_cache(maxsize=None)
def case(kind, a=0, b=0, l2=True):
    """One named case; a, b are its parameters (see CASES)."""
    near_tie = False
    if kind == "k":                                      # centroid count against the 64-row stage and the 4-stage ring
        rng = np.random.default_rng(_seed(1, a, l2))
        x, c = clustered(rng, 700, a, 1.0)
    elif kind == "bigk":                                 # the multi-stage stream at the shipped default, L2
        rng = np.random.default_rng(_seed(2, a))
        x, c = clustered(rng, 4096, a, 1.0)
    elif kind == "n":                                    # point count against the 32-point block, wave and 512-point tile
        rng = np.random.default_rng(_seed(3, a, l2))
        x, c = clustered(rng, a, 65, 1.0)
    elif kind == "negative":                             # every real score negative, k no multiple of 64
        rng = np.random.default_rng(_seed(4, a, l2))
        if l2:                                           # points far from every centroid: x.c << |c|^2/2
            c = (rng.standard_normal((a, D)) * (1 + rng.random((a, 1)))).astype(np.float32)
            x = (0.5 * rng.standard_normal((700, D))).astype(np.float16)
        else:
            c = -np.abs(rng.standard_normal((a, D))).astype(np.float32)
            x = np.abs(rng.standard_normal((700, D))).astype(np.float16)
    elif kind == "scale":                                # a = index into SCALES
        rng = np.random.default_rng(_seed(5, a, l2))
        x, c = clustered(rng, 700, 65, SCALES[a])
    elif kind == "twins":                                # every odd centroid a few fp16 ulps from its even neighbour
        rng = np.random.default_rng(_seed(6, a, l2))
        k = 128
        c = (TWIN_SCALES[a] * rng.standard_normal((k, D))).astype(np.float32)
        c[1::2] = c[0::2] * (1 + 2e-4 * rng.standard_normal((k // 2, 1)).astype(np.float32))
        c[5] = c[2]                                      # and one exact duplicate
        x = (c[rng.integers(0, k, 2000)] + 0.3 * TWIN_SCALES[a] * rng.standard_normal((2000, D))).astype(np.float16)
        near_tie = True
    elif kind == "old":                                  # the three shapes of test_kmeans_gpu.test_assign_matches_oracle
        n, k = a, b
        rng = np.random.default_rng(n + k)
        kc = max(k // 2, 2)
        centers = rng.standard_normal((kc, D)).astype(np.float32)
        x = (centers[rng.integers(0, kc, n)] + 0.15 * rng.standard_normal((n, D))).astype(np.float16)
        c = rng.standard_normal((k, D)).astype(np.float32) * (1 + rng.random((k, 1)).astype(np.float32))
    elif kind == "norm":                                 # L2 beyond |c| = 362, where -|c|^2/2 leaves fp16: a = |c|
        rng = np.random.default_rng(_seed(7, a))
        x, c = clustered(rng, 700, 65, a / np.sqrt(D))
    elif kind == "integers":                             # the `bad` data of test_clusering_never_rounds_float32_silently
        rng = np.random.default_rng(9)
        x = rng.integers(-2500, 2501, (2000, D)).astype(np.float32).astype(np.float16)
        g = rng.integers(0, 8, 2000)
        c = np.stack([x[g == j].astype(np.float32).mean(0) for j in range(8)] + [x[j].astype(np.float32) for j in range(5)])
        c = c.astype(np.float32)
    else:
        raise KeyError(kind)
    return x, c, l2, near_tie


SCALES = [1e-3, 0.05, 1.0, 25.0]
TWIN_SCALES = [1.0, 0.05]
K_SWEEP = [1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 321]
N_SWEEP = [1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1025]
OLD_SHAPES = [(3000, 37), (700, 64), (20000, 300)]
NORMS = [409, 523, 5000, 50000]

CASES = ([("k", k, 0, l2) for k in K_SWEEP for l2 in (True, False)] +
         [("bigk", 1500, 0, True), ("bigk", 10000, 0, True)] +
         [("n", n, 0, l2) for n in N_SWEEP for l2 in (True, False)] +
         [("negative", k, 0, l2) for k in (37, 65) for l2 in (True, False)] +
         [("scale", i, 0, l2) for i in range(len(SCALES)) for l2 in (True, False)] +
         [("twins", i, 0, l2) for i in range(len(TWIN_SCALES)) for l2 in (True, False)] +
         [("old", n, k, l2) for n, k in OLD_SHAPES for l2 in (True, False)] +
         [("norm", r, 0, True) for r in NORMS] +
         [("integers", 0, 0, True)])


def case_id(key):
    kind, a, b, l2 = key
    return f"{kind}-{a}" + (f"x{b}" if b else "") + ("-l2" if l2 else "-ip")


# ---- the float64 reference of a case (computed once, never modified) ---------------------------------------------------------

class Reference:
    def __init__(self, x, c, l2, near_tie):
        self.x, self.c, self.l2, self.near_tie = x, c, l2, near_tie
        n, k = len(x), len(c)
        x64, c64 = x.astype(np.float64), c.astype(np.float64)
        self.cc64 = (c64 ** 2).sum(1)
        self.xx64 = (x64 ** 2).sum(1)
        self.s64 = x64 @ c64.T - (0.5 * self.cc64[None] if l2 else 0.0)
        self.oracle_d, self.best = kmeans_oracle.assign(x, c, l2)
        self.best_s = self.s64[np.arange(n), self.best]
        assert (self.best_s >= self.s64.max(1) - 1e-12 * np.abs(self.best_s)).all()      # the oracle's own argmin / argmax
        if k > 1:
            top2 = -np.partition(-self.s64, 1, axis=1)[:, :2]
            self.lead = top2[:, 0] - top2[:, 1]
        else:
            self.lead = np.full(n, np.inf)
        hi, lo, h_stored = operand_format(c, l2)
        seen = hi.astype(np.float64) + lo.astype(np.float64)
        self.rep_c = float(np.sqrt(((c64 - seen) ** 2).sum(1)).max())
        self.rep_h = float(np.abs(-0.5 * self.cc64 - h_stored).max()) if l2 else 0.0
        self.xn = np.sqrt(self.xx64)
        self.c_max = float(np.sqrt(self.cc64.max()))
        self.units = self.xn * self.c_max + (0.5 * self.c_max ** 2 if l2 else 0.0)       # of the accumulation term
        self.tol = self.xn * self.rep_c + self.rep_h + GAMMA * self.units
        # bit-identical centroid rows: every index but the lowest of its group is banned
        _, first, inverse = np.unique(c.view(np.uint32).reshape(k, D), axis=0, return_index=True, return_inverse=True)
        self.banned = np.nonzero(first[inverse.reshape(-1)] != np.arange(k))[0]

    def near_tie_share(self):
        return float((self.lead < self.tol).mean())

    def float32_deviation(self):
        """Largest deviation of the plain float32 evaluation of the scores from float64, in units of the accumulation term."""
        x32, c32 = self.x.astype(np.float32), self.c.astype(np.float32)
        s32 = x32 @ c32.T
        if self.l2:
            s32 = s32 - np.float32(0.5) * (c32 * c32).sum(1, dtype=np.float32)[None]
        return float((np.abs(s32.astype(np.float64) - self.s64) / self.units[:, None]).max())


@functools.lru_cache(maxsize=None)
def reference(key):
    return Reference(*case(*key))


def check_against_float64(ref, labels, dist, where=None):
    """The rule of this file's header.  `where` restricts the check to a subset of the points (boolean mask)."""
    n, k = len(ref.x), len(ref.c)
    labels = np.asarray(labels).astype(np.int64)
    dist = np.asarray(dist).astype(np.float64)
    keep = np.ones(n, bool) if where is None else where
    assert labels.shape == (n,) and dist.shape == (n,)
    assert ((labels >= 0) & (labels < k))[keep].all(), "a label outside [0, k)"
    idx = np.nonzero(keep)[0]
    lab = labels[idx]
    assert not np.isin(lab, ref.banned).any(), "the higher index of two bit-identical centroids was returned"
    got_s = ref.s64[idx, lab]
    deficit = ref.best_s[idx] - got_s
    worst = int(np.argmax(deficit - ref.tol[idx]))
    assert (deficit <= ref.tol[idx]).all(), (
        f"{int((deficit > ref.tol[idx]).sum())} of {len(idx)} labels are worse than the float64 best by more than tol; point "
        f"{idx[worst]}: got {lab[worst]} (s64 {got_s[worst]!r}), best {ref.best[idx[worst]]} (s64 {ref.best_s[idx[worst]]!r}), "
        f"tol {ref.tol[idx[worst]]:.3e}; labels returned: {np.unique(labels)[:8]}")
    if ref.l2:
        want = np.maximum(ref.xx64[idx] - 2.0 * got_s, 0.0)
        allowed = 2.0 * ref.tol[idx] + 2.0 ** -24 * (ref.xx64[idx] + ref.cc64[lab])
    else:
        want = got_s
        allowed = 2.0 * ref.tol[idx] + 2.0 ** -24 * np.abs(got_s)
    err = np.abs(dist[idx] - want)
    worst = int(np.argmax(err - allowed)) if len(idx) else 0
    assert (err <= allowed).all(), (
        f"{int((~(err <= allowed)).sum())} of {len(idx)} distances are off by more than allowed; point {idx[worst]}: got "
        f"{dist[idx[worst]]!r}, float64 {want[worst]!r}, allowed {allowed[worst]:.3e}")
    return {"deficit/tol": float((deficit / ref.tol[idx]).max()) if len(idx) else 0.0,
            "dist err/allowed": float((err / allowed).max()) if len(idx) else 0.0,
            "differ from oracle": int((lab != ref.best[idx]).sum())}


def measure_reference_error(keys=None, verbose=True):
    """REFERENCE_DEVIATION and the table of this file's header, on the CPU: per case the float32 evaluation's deviation from
    float64 in units of the accumulation term, and the share of points whose float64 lead is below tol_i."""
    worst = 0.0
    rows = []
    for key in (CASES if keys is None else keys):
        ref = Reference(*case(*key))
        dev, share = ref.float32_deviation(), ref.near_tie_share()
        worst = max(worst, dev)
        rows.append((case_id(key), dev, share))
        if verbose:
            print(f"    {case_id(key):22s} deviation {dev:.2e}   share {100 * share:6.2f} %" + ("   (near-tie case)" if ref.near_tie else ""))
    if verbose:
        print(f"    REFERENCE_DEVIATION {worst:.3e}   GAMMA = 4 x = {4 * worst:.3e}   4e-5 / GAMMA = {NOMINATION_ALLOWANCE / (4 * worst):.1f}")
    return worst, rows


# ---- the three routes --------------------------------------------------------------------------------------------------------

def _lib():
    from proqa_amd import _lib as m
    return m, m.load()


class Handle:
    def __init__(self, n_max, k):
        self.m, self.lib = _lib()
        self.h = ctypes.c_void_p()
        self.m.check(self.lib.proqa_kmeans_create(D, int(n_max), int(k), ctypes.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.proqa_kmeans_free(self.h)

    def assign(self, x, c, l2, hint=None):
        import torch
        n = x.shape[0]
        lab = torch.full((n,), -7, dtype=torch.int32, device=x.device)
        dist = torch.full((n,), float("nan"), dtype=torch.float32, device=x.device)
        self.last = (lab, dist)
        self.m.check(self.lib.proqa_kmeans_assign_hinted_device(self.h, x.data_ptr(), n, c.data_ptr(), 1 if l2 else 0,
                                                                hint.data_ptr() if hint is not None else None, lab.data_ptr(),
                                                                dist.data_ptr(), self.m.current_stream_ptr()))
        torch.cuda.synchronize()
        return lab, dist

    def update(self, x, labels, k):
        import torch
        scratch = torch.zeros((k, D), dtype=torch.float32, device=x.device)
        counts = torch.zeros(k, dtype=torch.int32, device=x.device)
        self.m.check(self.lib.proqa_kmeans_update_device(self.h, x.data_ptr(), x.shape[0], labels.data_ptr(), scratch.data_ptr(),
                                                         counts.data_ptr(), self.m.current_stream_ptr()))
        return scratch, counts


def run_routes(x_np, c_np, l2, dev, hints=("right", "random", "out of range"), fixed_hint=None):
    """{route: (labels, distances)} as NumPy arrays."""
    import torch
    n, k = len(x_np), len(c_np)
    x = torch.from_numpy(x_np).to(dev)
    c = torch.from_numpy(c_np).to(dev)
    out = {}
    with Handle(n, k) as h:
        lab0, dist0 = h.assign(x, c, l2)
        out["two-pass"] = (lab0, dist0)
        h.update(x, lab0.clamp(0, k - 1), k)               # leaves the points' sorted order in the handle
        gen = torch.Generator().manual_seed(n * 31 + k)
        for name in hints:
            if name == "right":
                hint = lab0.clone()
            elif name == "random":
                hint = torch.randint(0, k, (n,), generator=gen, dtype=torch.int32).to(dev)
            elif name == "out of range":
                hint = torch.where(torch.arange(n, device=dev) % 2 == 0, k + 7, -1).to(torch.int32)
            else:
                hint = torch.full((n,), int(fixed_hint), dtype=torch.int32, device=dev)
            out["hinted, " + name] = h.assign(x, c, l2, hint)
    if n > 1:
        with Handle(n - 1, k) as h:
            out["full"] = h.assign(x, c, l2)
    else:                                                  # n_max < n needs two points: the same one twice
        with Handle(1, k) as h:
            lab, dist = h.assign(torch.cat([x, x]), c, l2)
            out["full"] = (lab[:1], dist[:1])
    return {name: (lab.cpu().numpy(), dist.cpu().numpy()) for name, (lab, dist) in out.items()}


def check_routes(ref, routes, where=None, report=None):
    keep = slice(None) if where is None else where
    first = routes["two-pass"][0]
    for name, (lab, dist) in routes.items():
        stats = check_against_float64(ref, lab, dist, where)
        print(f"    {report or ''} {name:22s} {stats}")
        assert np.array_equal(lab[keep], first[keep]), f"route '{name}' and the two-pass route return different labels"


# ---- the rule, tested on the CPU ---------------------------------------------------------------------------------------------

def test_the_rule_rejects_a_moved_label_and_a_shifted_distance():
    ref = reference(("k", 65, 0, True))
    n = len(ref.x)
    labels = ref.best.copy()
    got_s = ref.s64[np.arange(n), labels]
    dist = np.maximum(ref.xx64 - 2 * got_s, 0)
    check_against_float64(ref, labels, dist.astype(np.float32))
    far = int(np.argmax(ref.lead / ref.tol))                               # the point farthest from a tie
    assert ref.lead[far] > 100 * ref.tol[far]
    moved = labels.copy()
    moved[far] = int(np.argsort(-ref.s64[far])[1])                         # to its runner-up
    with pytest.raises(AssertionError, match="worse than the float64 best"):
        check_against_float64(ref, moved, dist)
    for sign in (1.0, -1.0):
        shifted = dist.copy()
        i = int(np.argmin(ref.xx64))
        shifted[i] += sign * (3 * ref.tol[i] + 2.0 ** -23 * (ref.xx64[i] + ref.cc64.max()))
        with pytest.raises(AssertionError, match="distances are off"):
            check_against_float64(ref, labels, shifted)
    with pytest.raises(AssertionError, match="outside"):
        check_against_float64(ref, np.where(np.arange(n) == 3, len(ref.c), labels), dist)
    twins = reference(("twins", 0, 0, True))
    lab_t = twins.best.copy()
    hit = np.nonzero(lab_t == 2)[0]
    assert len(hit) and list(twins.banned) == [5]
    lab_t[hit[0]] = 5                                                      # same score, higher index of the duplicate pair
    d_t = np.maximum(twins.xx64 - 2 * twins.s64[np.arange(len(lab_t)), lab_t], 0)
    with pytest.raises(AssertionError, match="bit-identical"):
        check_against_float64(twins, lab_t, d_t)


def test_the_measured_gamma_holds_for_the_small_cases_and_stays_below_the_nomination_allowance():
    assert GAMMA < NOMINATION_ALLOWANCE
    small = [key for key in CASES if key[0] in ("k", "n", "scale", "negative", "norm", "integers") and key[1] <= 700]
    worst, rows = measure_reference_error(small[::3], verbose=False)
    assert worst <= REFERENCE_DEVIATION, worst


def test_the_operand_format_carries_large_norms_exactly_and_small_ones_as_before():
    rng = np.random.default_rng(0)
    for norm in (1e-3, 0.5, 10.0, 181.0, 255.9, 256.1, 361.0, 409.0, 523.0, 5000.0, 65000.0):
        c = rng.standard_normal((40, D))
        c = (c * (norm / np.sqrt((c ** 2).sum(1)))[:, None]).astype(np.float32)
        hi, lo, stored = operand_format(c, True)
        seen = hi.astype(np.float64) + lo.astype(np.float64)
        h32 = (-0.5 * (seen ** 2).sum(1)).astype(np.float32).astype(np.float64)   # fp32 holds the norm; the five terms hold fp32
        assert np.isfinite(stored).all()
        assert (np.abs(stored - h32) <= 2.0 ** -22 * np.abs(h32) + 2.0 ** -24).all(), norm


# ---- on the device -----------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_assignment_against_float64_on_every_route(gpu_device, key):
    ref = reference(key)
    share = ref.near_tie_share()
    print(f"    {case_id(key)}: near-tie share {100 * share:.2f} %")
    if not ref.near_tie:
        assert share <= MAX_NEAR_TIE_SHARE, share
    if key[0] == "negative":
        assert (ref.s64 < 0).all() and len(ref.c) % 64                     # the zero padding rows would outscore every real one
    routes = run_routes(ref.x, ref.c, ref.l2, gpu_device)
    check_routes(ref, routes, report=case_id(key))
    if key[0] == "old":                                                    # the D tolerance test_assign_matches_oracle had
        np.testing.assert_allclose(routes["two-pass"][1], ref.oracle_d, rtol=2e-4, atol=2e-3)


def planted_case(order, l2):
    """c1 = sigma (1 + 0.45 ulp) is undersold by the hi-only pass by all of |x| |c1_lo| (x is parallel to its lo part), c2 =
    sigma with RAISED components one fp16 ulp up takes the hi-only lead; the fillers are fp16 numbers (lo = 0)."""
    rng = np.random.default_rng(77)
    sigma = np.where(rng.random(D) < 0.5, -1.0, 1.0)
    c1 = (sigma * (1 + 0.45 * 2.0 ** -10)).astype(np.float32)
    c2 = sigma.copy()
    c2[:RAISED] *= 1 + 2.0 ** -10
    fillers = np.where(rng.random((67, D)) < 0.5, -1.0, 1.0).astype(np.float32)
    c = fillers.copy()
    i1, i2 = (20, 41) if order == 0 else (41, 20)
    c[i1], c[i2] = c1, c2.astype(np.float32)
    x = np.tile((8 * sigma).astype(np.float16), (70, 1))
    x[1::2] = (fillers[rng.integers(0, 67, 35)] * 2).astype(np.float16)    # ordinary points in between
    return x, c, i1, i2


RAISED = 16


@gpu
@pytest.mark.parametrize("l2", [True, False], ids=["l2", "ip"])
@pytest.mark.parametrize("order", [0, 1])
def test_a_centroid_the_hi_pass_undersells_by_its_whole_bound_still_wins(gpu_device, order, l2):
    x, c, i1, i2 = planted_case(order, l2)
    ref = Reference(x, c, l2, True)
    hi, lo, h_stored = operand_format(c, l2)
    assert (lo[np.arange(len(c)) != i1] == 0).all() and (lo[i1] != 0).all()
    x64 = x[0].astype(np.float64)
    hi_only = hi.astype(np.float64) @ x64 + h_stored                       # what the nominating pass ranks by
    assert int(np.argmax(hi_only)) == i2
    assert int(ref.best[0]) == i1
    acc = GAMMA * ref.units[0]
    print(f"    float64 lead {ref.lead[0]:.4e} = {ref.lead[0] / acc:.0f} x the accumulation term; hi-only lead of the other "
          f"{hi_only[i2] - hi_only[i1]:.4e}")
    assert ref.lead[0] >= 100 * acc
    undersold = (c[i1].astype(np.float64) - hi[i1].astype(np.float64)) @ x64
    lo_norm = float(np.sqrt((lo[i1].astype(np.float64) ** 2).sum()))
    assert undersold >= 0.9 * ref.xn[0] * lo_norm
    routes = run_routes(x, c, l2, gpu_device, hints=("right", "random", "out of range", "the other"), fixed_hint=i2)
    check_routes(ref, routes)
    for name, (lab, _) in routes.items():
        assert (lab[0::2] == i1).all(), name


@gpu
def test_non_finite_points_leave_the_others_bit_identical(gpu_device):
    x, c, l2, _ = case("k", 65, 0, True)
    ref = reference(("k", 65, 0, True))
    dirty = x.copy()
    dirty[40, 7] = np.inf
    dirty[333] = np.nan
    clean = x.copy()
    clean[40] = 0
    clean[333] = 0
    others = np.ones(len(x), bool)
    others[[40, 333]] = False
    got, want = run_routes(dirty, c, l2, gpu_device), run_routes(clean, c, l2, gpu_device)
    for name in want:
        assert np.array_equal(got[name][0][others], want[name][0][others]), name
        assert np.array_equal(got[name][1][others].view(np.uint32), want[name][1][others].view(np.uint32)), name
        check_against_float64(ref, got[name][0], got[name][1], others)
        assert ((got[name][0] >= 0) & (got[name][0] < len(c))).all(), name      # the two bad points too: any valid label


@gpu
def test_centroids_beyond_the_supported_range_are_refused(gpu_device):
    import torch
    from proqa_amd._lib import ProqaError
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((100, D)).astype(np.float16)).to(gpu_device)
    ok = rng.standard_normal((9, D)).astype(np.float32)

    def attempt(c_np, l2, n_max=100):                                      # n_max = 50: the single full-precision pass
        with Handle(n_max, len(c_np)) as h:
            try:
                return h.assign(x, torch.from_numpy(c_np).to(gpu_device), l2)
            except ProqaError:
                torch.cuda.synchronize()
                assert (h.last[0] == -7).all() and torch.isnan(h.last[1]).all()          # refused: nothing written
                raise

    too_long = ok.copy()
    too_long[4] = 6000.0                                                   # |c| = 67 882 > 65504, every component an fp16 number
    for n_max in (100, 50):
        with pytest.raises(ProqaError, match="65504") as e:
            attempt(too_long, True, n_max)
        assert e.value.code == -1                                          # PROQA_EINVAL
    lab, dist = attempt(too_long, False)                                   # the inner product has no norm term: computed
    check_against_float64(Reference(x.cpu().numpy(), too_long, False, False), lab.cpu().numpy(), dist.cpu().numpy())
    for value in (70000.0, np.inf, -np.inf, np.nan):
        for l2 in (True, False):
            c_bad = ok.copy()
            c_bad[8, 127] = value
            with pytest.raises(ProqaError, match="65504"):
                attempt(c_bad, l2, 50 if value == 70000.0 else 100)
    lab, dist = attempt(ok, True)                                          # and an ordinary call right after is served
    check_against_float64(Reference(x.cpu().numpy(), ok, True, False), lab.cpu().numpy(), dist.cpu().numpy())


@gpu
def test_update_is_bit_identical_at_1500_centroids_and_planted_cluster_sizes(gpu_device):
    """proqa_kmeans_update_device with more than one counter per scan thread (k > 1024): cluster sizes of exactly 1, 31, 32,
    33, 63, 64, 65 and 200 among ordinary ones, some clusters empty."""
    import torch
    rng = np.random.default_rng(12)
    k = 1500
    sizes = rng.integers(2, 9, k)
    planted = {3: 1, 64: 31, 65: 32, 511: 33, 1023: 63, 1024: 64, 1025: 65, 1498: 200}
    empty = [0, 5, 700, 1026, 1499]
    for cl, s in planted.items():
        sizes[cl] = s
    sizes[empty] = 0
    a = rng.permutation(np.repeat(np.arange(k), sizes)).astype(np.int32)
    n = len(a)
    x = rng.standard_normal((n, D)).astype(np.float16)
    tx, ta = torch.from_numpy(x).to(gpu_device), torch.from_numpy(a).to(gpu_device)
    cent = torch.full((k, D), 7.0, dtype=torch.float32, device=gpu_device)
    m, lib = _lib()
    with Handle(n, k) as h:
        counts = torch.zeros(k, dtype=torch.int32, device=gpu_device)
        m.check(lib.proqa_kmeans_update_device(h.h, tx.data_ptr(), n, ta.data_ptr(), cent.data_ptr(), counts.data_ptr(),
                                               m.current_stream_ptr()))
        torch.cuda.synchronize()
    ref = np.zeros((k, D), np.float32)
    x32 = x.astype(np.float32)
    for i in range(n):                                                     # fp32 sums in point order, like the oracle's
        ref[a[i]] += x32[i]
    np.testing.assert_array_equal(counts.cpu().numpy(), sizes)
    filled = sizes > 0
    ref[filled] /= sizes[filled].astype(np.float32)[:, None]
    got = cent.cpu().numpy()
    np.testing.assert_array_equal(got[filled].view(np.uint32), ref[filled].view(np.uint32))
    assert (got[~filled] == 7.0).all()                                     # empty rows untouched


if __name__ == "__main__":
    measure_reference_error()
