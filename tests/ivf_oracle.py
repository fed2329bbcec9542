"""NumPy restatement of faiss 1.6.3 IndexIVFFlat(IndexFlatIP quantizer, d, nlist) -- TEST INFRASTRUCTURE ONLY.

The reference builds it at qa/online_sampler.py:75-79 (no metric argument: METRIC_L2) and searches it at :274.  faiss is
not installed here, so its source behaviour is restated:
  train   Level1Quantizer: Clustering(d, nlist), niter 10, max_points_per_centroid 256, seed 1234, assignment by the
          quantizer's inner product (oracle.kmeans_oracle.train(x, nlist, 10, 256, l2=False))
  add     every row to the list of its largest inner product with the centroids, ties to the lowest list, input order
  search  the nprobe lists of largest inner product (correctly rounded fp32 scores, ties to the lowest list), then the k
          rows of smallest sum (q - x)^2 among them, ties to the lowest id; the tail of a short result is I = -1,
          D = +FLT_MAX.
Distances are exact (float64, rounded once to float32).  A candidate enters the result only where `d < FLT_MAX` compares
true (faiss' heap starts at FLT_MAX and takes `dis < top`): rows holding +-inf or NaN are never returned.

The bound on D for rows that are not integers (distance_bound): with u = 2^-24 and D* the float64 distance,
  |D - D*| <= 2 GAMMA u sum|q_i x_i| + u |x|^2 + 2 u |s| + u |q|^2 + u |D*|
for the kernel's a = q.x (MFMA, fp32), h = fl(|x|^2 / 2), s = fl(a - h), n = fl(|q|^2), D = fl(n - 2 s): every term but
the first is one documented rounding.  GAMMA is 4 x the worst |a32 - q.x| / (u sum|q_i x_i|) of dot_kstep32, the float32
restatement of the dot product in the kernel's k-step order, over the float worlds below (192 queries x 2000 rows each;
measured on the CPU, recomputed by tests/test_ivf_host.py); the 4 is the allowance the project gives device sums over a
float32 restatement (tests/test_inbatch_gpu.py, K_INTRINSICS).

  world             worst |a32 - q.x| / (u sum|q_i x_i|)
  normal            1.857
  normal_x16        1.857
  near_duplicates   2.770
  GAMMA = 4 x 2.770 = 11.08

scan_model / merge_model restate the list protocol of ivf_scan and ivf_merge with switchable defects: what the integer worlds
of tests/test_ivf_edges_gpu.py would catch (tests/test_ivf_host.py runs the matrix).
"""
import numpy as np

from oracle import kmeans_oracle

FLT_MAX = np.float32(3.4028234663852886e38)
U = 2.0 ** -24
KSTEP_RATIO = {"normal": 1.857, "normal_x16": 1.857, "near_duplicates": 2.770}      # the table above
GAMMA = 4 * max(KSTEP_RATIO.values())


def train(x, nlist):
    """float32 centroids [nlist, d]"""
    cent, _ = kmeans_oracle.train(x, nlist, 10, 256, l2=False)
    return cent


def assign(x, centroids):
    """list of every row (int64 [n])"""
    return kmeans_oracle.assign(x, centroids, l2=False)[1]


def lists(assignment, nlist):
    """ids of every list in list order (= ascending id)"""
    return [np.nonzero(assignment == l)[0] for l in range(nlist)]


def coarse(xq, centroids, nprobe):
    """int64 [nq, min(nprobe, nlist)]: the probed lists, best first"""
    s = (np.asarray(xq, np.float32).astype(np.float64) @ np.asarray(centroids, np.float32).astype(np.float64).T).astype(np.float32)
    nlist = s.shape[1]
    order = np.lexsort((np.broadcast_to(np.arange(nlist), s.shape), -s.astype(np.float64)), axis=1)
    return order[:, :min(nprobe, nlist)]


def search(xq, xb, assignment, centroids, nprobe, k):
    """(D float32 [nq, k], I int64 [nq, k])"""
    xq64 = np.asarray(xq, np.float32).astype(np.float64)
    xb64 = np.asarray(xb, np.float32).astype(np.float64)
    nlist = centroids.shape[0]
    members = lists(assignment, nlist)
    probes = coarse(xq, centroids, nprobe)
    nq = xq64.shape[0]
    D = np.full((nq, k), FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        cand = np.concatenate([members[l] for l in probes[q]]) if probes.shape[1] else np.zeros(0, np.int64)
        if cand.size == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = ((xb64[cand] - xq64[q]) ** 2).sum(1)
            live = d.astype(np.float32) < FLT_MAX          # faiss' heap takes dis < top only: never NaN, never +inf
        cand, d = cand[live], d[live]
        order = np.lexsort((cand, d))[:k]
        D[q, :order.size] = d[order].astype(np.float32)
        I[q, :order.size] = cand[order]
    return D, I


def brute_l2(xq, xb, k):
    """exact L2 top-k over all rows (ties to the lowest id)"""
    xq64 = np.asarray(xq, np.float32).astype(np.float64)
    xb64 = np.asarray(xb, np.float32).astype(np.float64)
    nq = xq64.shape[0]
    D = np.full((nq, k), FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    ids = np.arange(xb64.shape[0])
    for q in range(nq):
        d = ((xb64 - xq64[q]) ** 2).sum(1)
        order = np.lexsort((ids, d))[:k]
        D[q, :order.size] = d[order].astype(np.float32)
        I[q, :order.size] = order
    return D, I


# ---------------------------------------------------------------------------------------------------------------------
# distances on non-integer rows: the bound on D
# ---------------------------------------------------------------------------------------------------------------------
def dot_kstep32(q, x):
    """float32 restatement of the scan's q.x: eight k-steps of 16 dimensions (pieces 2j, 2j + 1 at step j), the products of
    a step exact, their sum rounded to float32 and added to a float32 accumulator.  q [d], x [m, d] -> float32 [m]"""
    p = (np.asarray(x, np.float32).astype(np.float64) * np.asarray(q, np.float32).astype(np.float64)).reshape(len(x), 8, 16)
    acc = np.zeros(len(x), np.float32)
    for j in range(8):
        acc = acc + p[:, j].sum(1).astype(np.float32)        # float32 + float32: one rounding
    return acc


def kstep_ratio(xq, xb):
    """worst |dot_kstep32 - q.x| / (u sum |q_i x_i|) over all (query, row) pairs"""
    x64 = np.asarray(xb, np.float32).astype(np.float64)
    worst = 0.0
    for q in np.asarray(xq, np.float32).astype(np.float64):
        err = np.abs(dot_kstep32(q, xb).astype(np.float64) - x64 @ q)
        mag = np.abs(x64) @ np.abs(q)
        worst = max(worst, float((err[mag > 0] / (U * mag[mag > 0])).max()))
    return worst


def distance_bound(q, x):
    """bound on |D - D*| of the kernel's D = fl(n - 2 s), s = fl(a - h), a = q.x on the MFMA, h = fl(|x|^2 / 2),
    n = fl(|q|^2), against the float64 distance D*.  q [d], x [m, d] -> float64 [m]"""
    q64 = np.asarray(q, np.float32).astype(np.float64)
    x64 = np.asarray(x, np.float32).astype(np.float64)
    x2 = (x64 ** 2).sum(1)
    s = x64 @ q64 - x2 / 2
    d = ((x64 - q64) ** 2).sum(1)
    return 2 * GAMMA * U * (np.abs(x64) @ np.abs(q64)) + U * x2 + 2 * U * np.abs(s) + U * (q64 ** 2).sum() + U * d


def float_world(name):
    """(x fp16 [2000, 128], centroids float32 [8, 128], xq fp16 [192, 128]): 64 rows of the index, 64 rows moved by one fp16
    ulp on one coordinate, 64 fresh vectors"""
    rng = np.random.default_rng({"normal": 21, "normal_x16": 21, "near_duplicates": 23}[name])
    if name == "near_duplicates":
        centres = rng.standard_normal((25, 128)).astype(np.float32)
        x = (centres[rng.integers(0, 25, 2000)] + 2.0 ** -6 * rng.standard_normal((2000, 128)).astype(np.float32)).astype(np.float16)
        fresh = (centres[rng.integers(0, 25, 64)] + 2.0 ** -6 * rng.standard_normal((64, 128)).astype(np.float32)).astype(np.float16)
    else:
        x = rng.standard_normal((2000, 128)).astype(np.float16)
        fresh = rng.standard_normal((64, 128)).astype(np.float16)
    cent = rng.standard_normal((8, 128)).astype(np.float32)
    own = x[rng.choice(2000, 64, replace=False)].copy()
    moved = x[rng.choice(2000, 64, replace=False)].copy()
    cols = rng.integers(0, 128, 64)
    up = np.where(rng.integers(0, 2, 64) == 1, np.float16(np.inf), np.float16(-np.inf))
    moved[np.arange(64), cols] = np.nextafter(moved[np.arange(64), cols], up)
    xq = np.concatenate([own, moved, fresh])
    if name == "normal_x16":
        x, xq, cent = x * np.float16(16), xq * np.float16(16), cent * np.float32(16)
    return x, cent, xq


FLOAT_WORLDS = ("normal", "normal_x16", "near_duplicates")


# ---------------------------------------------------------------------------------------------------------------------
# integer worlds: every score exact in fp32
# ---------------------------------------------------------------------------------------------------------------------
def exact_in_fp32(xq, x, cent):
    """every partial sum of q.x, q.c, x.c and |q|^2 below 2^24, |x|^2 / 2 (a multiple of 1/2) below 2^23, all values
    integers: nothing the kernels compute for this world is rounded"""
    xq, x, cent = (np.asarray(v, np.float32).astype(np.float64) for v in (xq, x, cent))
    finite = x[np.isfinite(x).all(1)]
    whole = all((v == np.rint(v)).all() for v in (xq, finite, cent))
    big = max((np.abs(xq) @ np.abs(finite).T).max(), (np.abs(xq) @ np.abs(cent).T).max(), (np.abs(finite) @ np.abs(cent).T).max(),
              (xq ** 2).sum(1).max(), (finite ** 2).sum(1).max())
    return whole and big < 2.0 ** 24 and (finite ** 2).sum(1).max() / 2 < 2.0 ** 23


_TWO_SQUARES = {}


def _four_squares(m):
    """(a, b, c, d) >= 0 with a^2 + b^2 + c^2 + d^2 = m (Lagrange)"""
    if not _TWO_SQUARES:
        for a in range(200):
            for b in range(a, 200):
                _TWO_SQUARES.setdefault(a * a + b * b, (a, b))
    a = int(np.sqrt(m))
    while True:
        b = int(np.sqrt(m - a * a))
        while b >= 0:
            rest = m - a * a - b * b
            if rest in _TWO_SQUARES:
                return (a, b) + _TWO_SQUARES[rest]
            b -= 1
        a -= 1


def _offsets(m, rng):
    """int [n, 4] with squared norm m[i], random signs"""
    u = np.array([_four_squares(int(v)) for v in m], np.int64).reshape(len(m), 4)
    return u * rng.choice([-1, 1], u.shape)


LINE_ORDERS = ("ascending", "descending", "identical", "random", "mixed")


def line_world(n, order, nq=70, winners=(), seed=0, profile=None):
    """One list (nlist = 1) of n rows whose order by score is the same for every query.

    Row i = t + u_i: t small integers on dimensions 16.., u_i on dimensions 0..3 with |u_i|^2 = m_i.  A query is t plus
    -1..1 on dimensions 16.., so |q - x_i|^2 = m_i + (a constant of the query): m alone sets the order.
      ascending   m_i = n - 1 - i: every row beats all rows before it, for every query
      descending  m_i = i
      identical   every row is t
      random      m a permutation
      mixed       rows also carry -(i // 64), -(i % 64) on dimensions 4, 5 (m_i lowered by their squares), and the odd
                  queries 64, 1 there: even queries see n - 1 - i + const (ascending score), odd queries i + const
    profile: m itself, in place of the order's.
    winners: rows that are made the nearest of the list, row winners[j] for the queries q with q % (len + 1) == j (one-hot
    dimensions 8..): distance j there against >= 8 for every other row."""
    rng = np.random.default_rng(seed + 7919 * n + LINE_ORDERS.index(order))
    i = np.arange(n)
    t = np.zeros(128, np.int64)
    t[16:] = rng.integers(-2, 3, 112)
    x = np.tile(t, (n, 1))
    xq = np.tile(t, (nq, 1))
    xq[:, 16:] += rng.integers(-1, 2, (nq, 112))
    if order != "identical":
        p = {"ascending": n - 1 - i, "descending": i, "random": rng.permutation(n), "mixed": n - 1 - i}[order]
        if profile is not None:
            p = np.asarray(profile, np.int64)
        if winners:
            p = p + 10
            p[list(winners)] = np.arange(len(winners))
        if order == "mixed":
            x[:, 4], x[:, 5] = -(i // 64), -(i % 64)
            xq[1::2, 4], xq[1::2, 5] = 64, 1
            p = p + (n // 64) ** 2 + 63 ** 2 - (i // 64) ** 2 - (i % 64) ** 2
        x[:, :4] = _offsets(p, rng)
    for j, w in enumerate(winners):
        x[w, 8 + j] += 2
        xq[j::len(winners) + 1, 8 + j] += 2
    return x.astype(np.float16), np.ones((1, 128), np.float32), xq.astype(np.float16)


def plateau_profile():
    """640 rows, k = 128, for a schedule that appends the keys of a step in descending row order: rows 0..255 far, 256..383
    nearer and ascending (the first cut; the list is full again after it), 384..493 one tied score P that beats them all
    (second cut, 238 keys), 494..511 far, 512..639 P again: 18 of them fit (the highest ids), the third cut's k-th key is
    one of those, and the 110 left out tie with it at lower ids -- only `s >= tau` lets them back in"""
    i = np.arange(640)
    m = np.where(i < 256, 2000 + i, np.where(i < 384, 1383 - i, 5))
    m[494:512] = 3000 + i[494:512]
    return m


def merge_world(winners, seed=0):
    """64 lists of 130..170 rows, 40 queries that probe them all; `winners` = "last" or "first": where in a query's probe
    order its nearest rows sit.  Centroid l = (64 - l) e_l, row of list l = e_l + u (dimensions 64..67) + t; queries
    0..19 have 1 on dimensions 0..63 (probe order 0, 1, .., 63), the others 1 or 2 (orders of their own)."""
    rng = np.random.default_rng(seed + (winners == "first"))
    sizes = rng.integers(130, 171, 64)
    n = int(sizes.sum())
    lst = rng.permutation(np.repeat(np.arange(64), sizes))
    t = np.zeros(128, np.int64)
    t[72:] = rng.integers(-2, 3, 56)
    x = np.tile(t, (n, 1))
    x[np.arange(n), lst] = 1
    m = np.zeros(n, np.int64)
    for l in range(64):
        rows = np.nonzero(lst == l)[0]
        m[rows] = (63 - l if winners == "last" else l) * 40 + rng.permutation(len(rows))
    x[:, 64:68] = _offsets(m, rng)
    xq = np.tile(t, (40, 1))
    xq[:, 72:] += rng.integers(-1, 2, (40, 56))
    xq[:, :64] = 1
    xq[20:, :64] = rng.integers(1, 3, (20, 64))
    cent = np.zeros((64, 128), np.float32)
    cent[np.arange(64), np.arange(64)] = 64 - np.arange(64)
    return x.astype(np.float16), cent, xq.astype(np.float16)


def sign_world(seed=0):
    """nlist 4096: centroid l = the +-1 vector of l's 12 bits on dimensions 0..11; 12288 rows, each twice its list's
    centroid plus -2..2 on dimensions 12.. .  The lists with l % 16 == 7 stay empty.  Query 0 weighs dimensions 0..3 by 10
    against those lists' bits, so its best 1024 lists are all non-empty; the others are sign vectors with weights 1..3."""
    rng = np.random.default_rng(seed + 5)
    bits = 2 * ((np.arange(4096)[:, None] >> np.arange(12)) & 1) - 1
    cent = np.zeros((4096, 128), np.float32)
    cent[:, :12] = bits
    full = np.nonzero(np.arange(4096) % 16 != 7)[0]
    lst = rng.permutation(np.concatenate([np.repeat(full, 3), rng.choice(full, 12288 - 3 * len(full), replace=False)]))
    x = np.zeros((12288, 128), np.int64)
    x[:, :12] = 2 * bits[lst]
    x[:, 12:] = rng.integers(-2, 3, (12288, 116))
    xq = np.zeros((8, 128), np.int64)
    xq[:, :12] = bits[rng.integers(0, 4096, 8)] * rng.integers(1, 4, (8, 12))
    xq[0, :4] = [-10, -10, -10, 10]                     # bits 0..3 of 7 are 1, 1, 1, 0: the opposite signs
    xq[:, 12:] = rng.integers(-2, 3, (8, 116))
    return x.astype(np.float16), cent, xq.astype(np.float16)


def coarse_world(nlist, seed=0):
    """600 rows, each twice the centroid of a list drawn at random plus 0..2 (the first 30 all zero); non-negative
    centroids; from nlist 100 on lists 5 and 40 repeat the centroids of lists 2 and 17 and centroid 7 is zero; at nlist 3
    centroid 2 repeats centroid 0.  40 queries: a third <= 0 everywhere (every centroid score negative or zero), a third
    a centroid (the repeated ones and the zero one first) plus -1..1, a third -3..4"""
    rng = np.random.default_rng(seed + 31 * nlist)
    cent = rng.integers(0, 4, (nlist, 128)).astype(np.float32)
    if nlist == 3:
        cent[2] = cent[0]
    if nlist >= 100:
        cent[5], cent[40], cent[7] = cent[2], cent[17], 0
    x = 2 * cent[rng.integers(0, nlist, 600)].astype(np.int64) + rng.integers(0, 3, (600, 128))
    x[:30] = 0
    xq = rng.integers(-3, 5, (40, 128))
    xq[::3] = -rng.integers(0, 4, (len(xq[::3]), 128))
    aim = np.concatenate([[2, 5, 17, 40, 7], rng.integers(0, nlist, 8)]) % nlist
    xq[1::3] = cent[aim].astype(np.int64) + rng.integers(-1, 2, (13, 128))
    return x.astype(np.float16), cent, xq.astype(np.float16)


def nonfinite_world(seed=0):
    """nlist 4: 40 finite integer rows in list 0, 60 in each other list, then three rows of list 0's shape holding +inf,
    -inf and NaN (ids 220, 221, 222).  Centroid columns 20 and 21 send the infinite rows to list 0.  Queries 0..7 aim at
    list 0, with -1, 0 or 1 on the dimensions of the non-finite values: q.x there is -inf, NaN or +inf."""
    rng = np.random.default_rng(seed + 77)
    lst = np.repeat(np.arange(4), [40, 60, 60, 60])
    x = rng.integers(-2, 3, (223, 128)).astype(np.float32)
    x[:, :4] = 0
    x[:, 20:23] = 0
    x[np.arange(220), lst] = 6
    x[220:, 0] = 6
    x[220, 20], x[221, 21], x[222, 22] = np.inf, -np.inf, np.nan
    cent = np.zeros((4, 128), np.float32)
    cent[np.arange(4), np.arange(4)] = 1
    cent[:, 20], cent[:, 21] = -1, 1
    cent[0, 20], cent[0, 21] = 1, -1
    xq = rng.integers(-2, 3, (20, 128)).astype(np.float32)
    xq[:, :4] = 0
    xq[np.arange(20), np.concatenate([np.zeros(8, np.int64), rng.integers(1, 4, 12)])] = 9
    xq[:, 20:23] = rng.integers(-1, 2, (20, 3))
    xq[0, 20:23], xq[1, 20:23], xq[2, 20:23] = (-1, 1, -1), (1, -1, 1), (0, 0, 0)
    return x.astype(np.float16), cent, xq.astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------------
# the list protocol of ivf_scan and ivf_merge, with switchable defects
# ---------------------------------------------------------------------------------------------------------------------
SCAN_DEFECTS = ("drop_left_out", "strict_tau", "cut_keeps_k_minus_1", "refuse_at_255", "clamped_tail")
MERGE_DEFECTS = ("skip_first_of_batch", "ge_kth")
_RUN = 256          # keys of one running list
_STEP = 128         # rows of one step: four tiles of 32
_MERGE_KEYS = 4096


def pack_keys(score, ids):
    """(ord(score) << 32) | (0xFFFFFFFF - id): descending key = score descending, id ascending; -0.0 ties with +0.0"""
    u = np.asarray(score, np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, np.uint64(0), u)
    o = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return (o << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(ids).astype(np.uint64))


def unpack_keys(keys):
    """(score float32, id int64) of keys"""
    keys = np.asarray(keys, np.uint64)
    o = (keys >> np.uint64(32)).astype(np.uint32)
    u = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o)
    return u.astype(np.uint32).view(np.float32), (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)


def scan_model(scores, ids, k, defect=None, trace=None, reverse_steps=False):
    """One scan work item: float32 scores [Q, n] of Q <= 32 queries against the n rows of a chunk, ids [n].  Rows arrive in
    steps of 128; a key enters a query's list of 256 when s >= tau and key > k-th key (both as of the last cut); a step in
    which any list ran over cuts every list to its best k and appends the keys left out again; a last cut, a sort.
    Within a step the GPU appends in no fixed order; the model appends in row order, or with reverse_steps in descending
    row order.  Non-finite scores never pass: tau starts at -FLT_MAX.  `trace`, a dict, receives the number of cuts and the longest
    list seen after an append of left-out keys.
    -> uint64 [Q, k] sorted keys, 0 where the list is short."""
    assert defect is None or defect in SCAN_DEFECTS
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids, np.int64)
    Q, n = scores.shape
    if defect == "clamped_tail" and n % 32:
        pad = 32 - n % 32
        scores = np.concatenate([scores, np.repeat(scores[:, -1:], pad, 1)], 1)
        ids = np.concatenate([ids, np.repeat(ids[-1:], pad)])
        n += pad
    keys = pack_keys(scores, ids[None])
    run = [np.zeros(0, np.uint64) for _ in range(Q)]
    tau = np.full(Q, -FLT_MAX, np.float32)
    kth = np.zeros(Q, np.uint64)

    def cut(q, keep):
        srt = np.sort(run[q])[::-1]
        if len(srt) >= k:
            kth[q] = srt[k - 1]
            tau[q] = unpack_keys(srt[k - 1:k])[0][0]
        run[q] = srt[:keep]

    for r0 in range(0, n, _STEP):
        sc, ky = scores[:, r0:r0 + _STEP], keys[:, r0:r0 + _STEP]
        if reverse_steps:
            sc, ky = sc[:, ::-1], ky[:, ::-1]
        with np.errstate(invalid="ignore"):
            passed = ((sc > tau[:, None]) if defect == "strict_tau" else (sc >= tau[:, None])) & (ky > kth[:, None])
        left = []
        for q in range(Q):
            new = ky[q][passed[q]]
            room = _RUN - len(run[q])
            run[q] = np.concatenate([run[q], new[:room]])
            left.append((sc[q][passed[q]][room:], new[room:]))
        if any(len(l[1]) for l in left):
            for q in range(Q):
                cut(q, k - 1 if defect == "cut_keeps_k_minus_1" else k)
                if defect == "drop_left_out":
                    continue
                s_l, k_l = left[q]
                again = k_l[((s_l > tau[q]) if defect == "strict_tau" else (s_l >= tau[q])) & (k_l > kth[q])]
                cap = _RUN - 1 if defect == "refuse_at_255" else _RUN
                run[q] = np.concatenate([run[q], again])[:cap]
                if trace is not None:
                    trace["longest_after_reappend"] = max(trace.get("longest_after_reappend", 0), len(run[q]))
            if trace is not None:
                trace["cuts"] = trace.get("cuts", 0) + 1
    out = np.zeros((Q, k), np.uint64)
    for q in range(Q):
        cut(q, k)
        out[q, :len(run[q])] = run[q]
    return out


def merge_model(partials, k, defect=None):
    """One query's merge: partials uint64 [n_lists, k] (0 = no key) in batches of (4096 - k) // k lists; a key enters the
    sort when it is above the running k-th key.  -> (uint64 [k] sorted keys, number of live keys)"""
    assert defect is None or defect in MERGE_DEFECTS
    partials = np.asarray(partials, np.uint64).reshape(-1, k)
    per_batch = (_MERGE_KEYS - k) // k
    run = np.zeros(0, np.uint64)
    kth = np.uint64(0)
    for f0 in range(0, len(partials), per_batch):
        lo = f0 + 1 if defect == "skip_first_of_batch" and f0 else f0
        batch = partials[lo:f0 + per_batch].reshape(-1)
        new = batch[batch >= kth] if defect == "ge_kth" else batch[batch > kth]
        if len(new):
            run = np.sort(np.concatenate([run, new]))[::-1][:k]
            if len(run) == k:
                kth = run[k - 1]
    out = np.zeros(k, np.uint64)
    out[:len(run)] = run
    return out, len(run)


def model_search(xq, xb, assignment, centroids, nprobe, k, scan_defect=None, merge_defect=None, chunk=4096, trace=None, reverse_steps=False):
    """The whole search on the two models: work items of (list, chunk of its rows, 32 of its queries in query order), the
    partial lists of a query merged in probe order.  -> (D, I) as search() gives them"""
    xq64 = np.asarray(xq, np.float32).astype(np.float64)
    xb64 = np.asarray(xb, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        hn = ((xb64 ** 2).sum(1) / 2).astype(np.float32)
    nlist = centroids.shape[0]
    members = lists(assignment, nlist)
    probes = coarse(xq, centroids, nprobe)
    nq = len(xq64)
    partial = {}
    for l in range(nlist):
        qs = np.nonzero((probes == l).any(1))[0]
        if not len(qs) or not len(members[l]):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            sc = (xq64[qs] @ xb64[members[l]].T).astype(np.float32) - hn[members[l]][None]
        for q0 in range(0, len(qs), 32):
            for c, r0 in enumerate(range(0, len(members[l]), chunk)):
                out = scan_model(sc[q0:q0 + 32, r0:r0 + chunk], members[l][r0:r0 + chunk], k, scan_defect, trace, reverse_steps)
                for j, q in enumerate(qs[q0:q0 + 32]):
                    partial[(int(q), l, c)] = out[j]
    D = np.full((nq, k), FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        mine = [partial[(q, l, c)] for l in probes[q] for c in range(-(-len(members[l]) // chunk)) if (q, l, c) in partial]
        if not mine:
            continue
        keys, live = merge_model(np.stack(mine), k, merge_defect)
        s, ids = unpack_keys(keys[:live])
        with np.errstate(invalid="ignore", over="ignore"):
            D[q, :live] = ((xq64[q] ** 2).sum().astype(np.float32).astype(np.float64) - 2.0 * s.astype(np.float64)).astype(np.float32)
        I[q, :live] = ids
    return D, I


# ---------------------------------------------------------------------------------------------------------------------
# the catalogue of integer worlds: name -> (builder, nprobe values, k values)
# ---------------------------------------------------------------------------------------------------------------------
LINE_ROWS = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 383, 384, 385, 640, 4095, 4096, 4097)
LINE_KS = (1, 2, 5, 80, 127, 128)
LINE_NQS = (1, 31, 32, 33, 70)
CHUNK_EDGE_ROWS = (4095, 4096, 8191, 8192, 8999)
COARSE_NLISTS = (1, 2, 3, 100, 257)


def integer_worlds():
    worlds = {}
    for order in LINE_ORDERS:
        for n in LINE_ROWS:
            worlds[f"line-{order}-{n}"] = (lambda n=n, order=order: line_world(n, order), (1,), LINE_KS)
    worlds["line-plateau-640"] = (lambda: line_world(640, "random", profile=plateau_profile()), (1,), (128, 80, 5))
    for order in ("ascending", "descending", "random"):
        worlds[f"chunks-{order}"] = (lambda order=order: line_world(9000, order), (1,), (1, 80, 128))
    worlds["chunks-edges"] = (lambda: line_world(9000, "descending", winners=CHUNK_EDGE_ROWS), (1,), (1, 80, 128))
    for winners in ("last", "first"):
        worlds[f"merge-{winners}"] = (lambda winners=winners: merge_world(winners), (64,), (128, 80, 1))
    worlds["sign"] = (sign_world, (1024,), (5, 128))
    for nlist in COARSE_NLISTS:
        worlds[f"coarse-{nlist}"] = (lambda nlist=nlist: coarse_world(nlist), (1, nlist, nlist + 5), (5, 128))
    return worlds
