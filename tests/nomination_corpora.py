"""Corpora whose planted rows sit at the edge of the int8 nomination bound -- TEST INFRASTRUCTURE ONLY (CPU constructions,
shared by test_nomination_oracle_host.py and test_nomination_edges_gpu.py; the quantiser and the bound: nomination_oracle.py).

Everything lives on power-of-two grids, so that every row and query is an exact fp16 number, the quantiser's float32
arithmetic is exact, and every partial sum of every dot product fits 24 bits (asserted by the host test): the float64
oracle's score bits are the only right ones.

    row of a block of LEVEL j     x_d = mean_d + c_d 2^-j (xi_d + r_d) / 128,   c_d a power of two, max |xi| = 127 in every block
                                  => f_b = (127 / 128) 2^-j, G_b = 128 2^j, and xi, r are what the quantiser finds, exactly
    the shard's scale rows        x_d = mean_d +- c_d in one dimension each (blocks 0..7: they make c_d what it is; f_b = 1)
    edge query                    q_d = n_d / (16 c_d), n_d = 16 qi_d + 16 e_d an integer, n_127 = 16 * 127 => s_q = 1 exactly
    score                         q.x - q.mean = 2^-j / 128 * sum_d (n_d / 16) (xi_d + r_d)

Column sums are zero by construction (mean_d is exact): background rows come in antithetic pairs, edge queries come in pairs
(q, -q) whose planted rows and anchors are each other's negatives.  A background row carries xi_0 = +-127 (the block's
maximum; edge queries weigh dimension 0 with qi = 1) and small entries elsewhere, the same absolute size at every level.

Per edge query: ONE planted row behind the bootstrap, scoring T + eps (eps below one integer unit of its block), and 128
ANCHOR rows inside the first 4096 rows that all score exactly T (on the int8 grid: r = 0; found by solving n.xi = N; they
differ from each other in directions their query does not see, so that no other query finds 128 tied rows).
No other row reaches T (host test), so the running threshold of an edge query is T in every round, for every k <= 128.
What the planted row tests is the GAP between the real threshold and its integer score,
    gap = (T - q.mean) G_b / s_q - acc = shortfall - eps,     as a fraction of bound = ||w / s_q|| R + ||e|| X_b:
a scan whose margin is narrower than that fraction of the rigorous one loses the row.

    B rows   query with e = 0 (qi = +-127, qi_0 = 1); row xi = a sign(q) plus r_d = 7/16 sign(q_d) on m dimensions:
             shortfall = 127 * 7/16 * m against ||qi|| R, R = 7/16 sqrt(m_max): fraction m / sqrt(127 m_max), the top rung
             (m = m_max) is the Cauchy-Schwarz equality case
    E rows   query with qi = +-126 and e_d = +-7/16, aligned with qi on m dimensions; row xi = a sign(qi) on the grid and the
             largest-norm row of its block: shortfall = 7/16 a (2 m - L + 2) against ||e|| X_b = 7/16 a (L + 2)
    BE rows  both at once, with r_d = 1/4 (odd sixteenths times odd sixteenths would not fit 24 bits at a useful size)
A corpus holds rows of ONE kind: an E query's bound carries ||w / s_q|| R, which rows with residuals would make the larger
term.  The sign patterns of the pairs are rows of a Hadamard matrix: a pair's rows score ~ 0 for the other pairs."""
import numpy as np

DIM = 128
BLOCK = 32
BOOT = 4096
ANCHORS = 128
SCALE_BLOCKS = 8
ANCHOR_BLOCKS_PER_QUERY = 5
ANCHORS_PER_BLOCK = 26
DECOY_BLOCK = 560                    # decoy rows: row 9 of blocks 560, 563, 566, ...
RUNGS = (0.5, 0.75, 0.9, 0.97, 0.995)
N_ROWS = 20011                       # 625 blocks and 11 rows: several rounds behind the bootstrap, a partial last block
N_WIDE = 200011                      # 6250 blocks and 11 rows: the last slab's chunks hold 3 or 4 stages (hetero_wide)
CUS = 256                            # compute units of the MI355X: the chunk geometry below is that device's


def plan(n, nq, k, cus=CUS, boot=BOOT):
    """[(first row, end row, rows_per_chunk)] of the int8 rounds behind the bootstrap, leaps off, default schedule: what
    mips_index.cpp derives (growth_for, plan_slabs_equal, and run_round's geometry for a nominating round: slabs of equal
    growth, at least max(64, 2 CUs / query tiles) chunks per slab, chunks of whole 128-row stages).  A chunk starts at
    first row + i * rows_per_chunk; its 32-row units 0..3 are stage 0, units 0..7 pair 0, units 8.. pair 1."""
    import math
    qw = 2 if nq > 256 else 1
    n_qtiles = -(-nq // (256 * qw))
    growth = min(6.0 if qw == 1 else 2.0, 640.0 / k)
    ratio = n / boot
    rounds = max(1, math.ceil(math.log(ratio) / math.log(1.0 + growth) - 1e-9))
    step = ratio ** (1.0 / rounds)
    target = max(64, (2 * cus // n_qtiles) // 8 * 8, (cus // n_qtiles) // 8 * 8)
    out, seen = [], boot
    for r in range(rounds):
        if seen >= n:
            break
        r1 = n if r + 1 == rounds else -(-int(boot * step ** (r + 1)) // 128) * 128
        r1 = min(n, max(r1, seen + 128))
        out.append((seen, r1, -(-(-(-(r1 - seen) // target)) // 128) * 128))
        seen = r1
    if seen < n:
        out.append((seen, n, -(-(-(-(n - seen) // target)) // 128) * 128))
    return out


class Corpus:
    pass


def _amp(level):
    return max(1, 2 ** (level - 1))


def _signs(h):
    """row h of the Sylvester-Hadamard matrix of order 128, made positive in dimension 127: the sign patterns of two pairs are
    orthogonal, so that one pair's anchors and planted row score next to nothing for every other pair (levels differ by
    up to 16 x in absolute size)"""
    d = np.arange(DIM)
    row = np.array([1 - 2 * (bin(h & int(x)).count("1") & 1) for x in d])
    return row * row[127]


def _edge_vectors(kind, rung, rng, big, quiet_sign, a, h):
    """(n, Y) of the +q member of a pair: n_d = 16 (qi_d + e_d), Y_d = 16 (xi_d + r_d) of its planted row"""
    n = np.zeros(DIM, np.int64)
    Y = np.zeros(DIM, np.int64)
    frac = RUNGS[rung]
    n[0], n[127] = 16, 16 * 127
    for d, s in quiet_sign.items():
        n[d] = 16 * 127 * s
    if kind == "B":
        dims = np.array([d for d in [1, 2] + list(big)])
        sig = _signs(h)[dims]
        n[dims] = 16 * 127 * sig
        res = np.concatenate([dims, [127]])
        Y[res] = 16 * a * np.sign(n[res])
        L = len(res)
        # fraction m / sqrt(||qi||^2 / 127^2 * m_max), m_max = L (every B corpus holds a top rung); the top rung takes all
        m = L if rung == len(RUNGS) - 1 else int(np.ceil(frac * np.sqrt(L * (L + len(quiet_sign) + 1e-3)))) + 1
        pick = rng.permutation(res)[:min(m, L)]
        Y[pick] += 7 * np.sign(n[pick])
        return n, Y
    dims = np.array(list(big))
    L = len(dims)
    sig = _signs(h)[dims]
    m = L if rung == len(RUNGS) - 1 else int(np.ceil((frac * (L + 2) + L - 2) / 2.0))
    al = np.where(rng.permutation(L) < min(m, L), 1, -1)           # e aligned with qi on m dimensions
    n[dims] = 16 * 126 * sig + 7 * sig * al
    n[1], n[2] = 7, 9                                              # (qi, e) = (0, +7/16) and (1, -7/16)
    Y[dims] = 16 * a * sig
    Y[1], Y[2] = 16 * a, -16 * a
    if kind == "BE":
        res = np.concatenate([dims, [127]])
        mr = len(res) if rung == len(RUNGS) - 1 else int(np.ceil(frac * len(res))) + 1
        pick = rng.permutation(res)[:min(mr, len(res))]
        Y[pick] += 4 * np.sign(n[pick])                            # r = 1/4: odd sixteenths times odd sixteenths would not fit 24 bits
    return n, Y


def _anchor(kind, n, Y, big, below=0):
    """an int8-grid row xi with 16 n.xi = the largest reachable value below the planted row's n.Y (`below`: that many
    integer units of a B query further down: a decoy)"""
    V = int(n @ Y)
    N = 16 * (-(-V // 256) - 1 - below) if kind == "B" else -(-V // 16) - 1
    xi = np.sign(Y) * (np.abs(Y) // 16)
    delta = N - int(n @ xi)
    for _ in range(64):
        if abs(delta) < 1100:
            break
        for d in big:
            if abs(delta) < 1100:
                break
            step = int(np.sign(delta) * np.sign(n[d]))
            xi[d] += step
            delta -= step * int(n[d])
    if kind == "B":
        assert delta % 16 == 0
        xi[0] += delta // 16
    else:
        best = None
        for x1 in range(-8, 9):
            for x2 in range(-8, 9):
                rest = delta - 7 * x1 - 9 * x2
                if rest % 16 == 0 and (best is None or abs(x1) + abs(x2) < best[0]):
                    best = (abs(x1) + abs(x2), x1, x2, rest // 16)
        xi[1] += best[1]
        xi[2] += best[2]
        xi[0] += best[3]
    assert int(n @ xi) == N and np.abs(xi).max() <= 127 and 16 * N < V
    return 16 * xi


def build(name, pairs, levels=None, default_level=3, a=None, c_exp=None, quiet=None, const_dims=(), zero_query=False,
          fat=(), h0=3, decoys=(), n_rows=N_ROWS, seed=0):
    """pairs: [(kind, rung, (block, pos) of +q's planted row, (block, pos) of -q's)]; levels: {block: level}; fat: blocks
    whose two neighbours get a row of |xi| = 124 in every dimension (norm 1403: their X_b), +- a Hadamard pattern no edge
    query uses; decoys: fractions f of the B bound -- each of the first len(decoys) pairs (B rows, every rung present) gets a
    row on the int8 grid that scores T - f * bound for +q (and its negative for -q): below T, so never in a result, but
    forced for f < 1, outside allowed for f > 1 + the kernel's inflation, in the band between the two just above 1"""
    rng = np.random.default_rng(seed)
    a = dict({"B": 48, "E": 64, "BE": 16}, **(a or {}))
    quiet = quiet or {}                                            # {dim: mean_d / c_d}: rows stay at the mean there
    nb = (n_rows + BLOCK - 1) // BLOCK
    level = np.full(nb, default_level, np.int64)
    for b, j in (levels or {}).items():
        level[b] = j
    big = [d for d in range(3, 127) if d not in quiet and d not in const_dims]
    live = [d for d in range(1, DIM) if d not in quiet and d not in const_dims]
    Y = np.zeros((n_rows, DIM), np.int64)
    taken = np.zeros(n_rows, bool)
    taken[:SCALE_BLOCKS * BLOCK] = True
    ns, planted, kinds, rungs, decoy_rows = [], [], [], [], []
    assert 2 * len(pairs) * ANCHOR_BLOCKS_PER_QUERY <= BOOT // BLOCK - SCALE_BLOCKS
    for t, (kind, rung, slot_p, slot_m) in enumerate(pairs):
        n, y = _edge_vectors(kind, rung, rng, big, {d: int(np.sign(v)) for d, v in quiet.items()}, a[kind], 5 * t + h0)
        anchor = _anchor(kind, n, y, big)
        # the 128 anchors differ from each other by vectors the query does not see (+-1, +-2, +-3 on two dimensions of equal
        # |n_d|): one score T for their own query, distinct scores for every other one
        twists = np.zeros((ANCHORS, DIM), np.int64)
        groups = [[d for d in big if abs(n[d]) == v] for v in sorted({abs(int(n[d])) for d in big})]
        duo = [(g[2 * j], g[2 * j + 1]) for g in groups for j in range(len(g) // 2)]
        for cpy in range(ANCHORS):
            d1, d2 = duo[cpy % len(duo)]
            mult = 1 + cpy // len(duo)
            twists[cpy, d1], twists[cpy, d2] = mult * np.sign(n[d1]), -mult * np.sign(n[d2])
        assert not (twists @ n).any() and np.abs(anchor // 16 + twists).max() <= 127
        assert level[slot_p[0]] == level[slot_m[0]]
        for sgn, (b, pos) in ((1, slot_p), (-1, slot_m)):
            i = len(ns)
            row = b * BLOCK + pos
            assert BOOT <= row < n_rows and not taken[row]
            Y[row], taken[row] = sgn * y, True
            b0 = SCALE_BLOCKS + ANCHOR_BLOCKS_PER_QUERY * i
            level[b0:b0 + ANCHOR_BLOCKS_PER_QUERY] = level[b]
            left = ANCHORS
            for ab in range(b0, b0 + ANCHOR_BLOCKS_PER_QUERY):
                cnt = min(left, ANCHORS_PER_BLOCK)
                # (the anchors' positions in their block rotate with the query)
                rows_ = ab * BLOCK + (np.arange(cnt) + 5 * i) % BLOCK
                Y[rows_], taken[rows_] = sgn * (anchor + 16 * twists[ANCHORS - left:ANCHORS - left + cnt]), True
                left -= cnt
            if t < len(decoys):
                assert kind == "B"
                L = len(big) + 3                       # dimensions with a residual on the top rung: R = 7/16 sqrt(L)
                bound = np.sqrt(127.0 ** 2 * (L + len(quiet)) + 1.0) * 7.0 / 16.0 * np.sqrt(L)
                drow = (DECOY_BLOCK + 6 * t + 3 * (sgn < 0)) * BLOCK + 9
                assert not taken[drow] and level[drow // BLOCK] == level[b]
                Y[drow], taken[drow] = sgn * _anchor(kind, n, y, big, below=int(round(decoys[t] * bound))), True
                decoy_rows.append(drow)
            ns.append(sgn * n)
            planted.append(row)
            kinds.append(kind)
            rungs.append(rung)
    for t, b in enumerate(fat):
        assert level[b - 1] == level[b + 1]
        for sgn, nbk in ((1, b - 1), (-1, b + 1)):
            row = nbk * BLOCK + int(np.flatnonzero(~taken[nbk * BLOCK:(nbk + 1) * BLOCK])[-1])
            keep = np.zeros(DIM, np.int64)
            keep[[0] + live] = 1
            Y[row], taken[row] = sgn * 16 * 124 * _signs(127 - t) * keep, True
    # background: antithetic pairs inside a level
    free = np.flatnonzero(~taken)
    for j in np.unique(level):
        rows_ = rng.permutation(free[level[free // BLOCK] == j])
        half = len(rows_) // 2
        amp = _amp(int(j))
        if amp == 1:
            xi = rng.integers(-1, 2, (half, DIM)) * (rng.random((half, DIM)) < 0.25)
        else:
            xi = rng.integers(-amp, amp + 1, (half, DIM))
        keep = np.zeros(DIM, bool)
        keep[live] = True
        xi = xi * keep
        xi[:, 0] = 127
        Y[rows_[:half]] = 16 * xi
        Y[rows_[half:2 * half]] = -16 * xi                         # (an odd row out stays at the mean)
    # the rows as real numbers, in units of c_d
    U = Y.astype(np.float64) * (2.0 ** -level[np.arange(n_rows) // BLOCK].astype(np.float64))[:, None] / 2048.0
    for d in range(DIM):
        if d not in const_dims:
            U[2 * d, d], U[2 * d + 1, d] = 1.0, -1.0
    c = 16.0 * 2.0 ** (np.zeros(DIM) if c_exp is None else np.asarray(c_exp, np.float64))
    mean = np.zeros(DIM)
    for d, v in quiet.items():
        mean[d] = v * c[d]
    for d in const_dims:
        mean[d] = 0.5 * (d % 3 + 1)
    x = mean + c * U
    xb = x.astype(np.float16)
    assert (xb.astype(np.float64) == x).all(), "a row is not an exact fp16 number"
    assert np.abs(x.sum(axis=0) - n_rows * mean).max() == 0.0, "column sums: the mean is not exact"
    ns = np.array(ns)
    q = ns / 16.0 / c
    q[:, list(const_dims)] = 1.0                                   # (no weight in the scan: its whole share is q.mean)
    edge_q = q.astype(np.float16)
    assert (edge_q.astype(np.float64) == q).all(), "an edge query is not an exact fp16 number"
    plain = 16 * rng.integers(-40, 41, (64, DIM)) / 16.0 / c
    plain_q = plain.astype(np.float16)
    assert (plain_q.astype(np.float64) == plain).all()

    cp = Corpus()
    cp.name, cp.xb, cp.edge_q, cp.plain_q = name, xb, edge_q, plain_q
    cp.extra_q = np.zeros((1, DIM), np.float16) if zero_query else np.zeros((0, DIM), np.float16)
    cp.planted = np.array(planted)
    cp.decoy_rows, cp.decoys = np.array(decoy_rows, np.int64), tuple(decoys)      # (two rows per fraction: +q's, -q's)
    cp.kinds, cp.rungs = kinds, np.array(rungs)
    cp.declared = np.array([RUNGS[r] for r in rungs])
    cp.level = level
    x64 = xb.astype(np.float64)
    S_boot = edge_q.astype(np.float64) @ x64[:BOOT].T
    cp.T = np.sort(S_boot, axis=1)[:, -ANCHORS]                    # the 128th best of the first 4096 rows: the anchors' score
    cp.planted_score = np.einsum("ij,ij->i", edge_q.astype(np.float64), x64[cp.planted])
    return cp


def batch(cp, nq, rotate=0, fill="plain", zero=False):
    """(xq [nq, 128], pos = {lane: edge query}): edge queries in the first and last lanes of the 32-query blocks (query
    `rotate` first), the rest plain queries; zero = True puts the corpus's all-zero query into lane 1.  fill = "edge": the edge
    queries over and over -- every query of the batch then keeps the threshold T of its edge query in every round"""
    ne = len(cp.edge_q)
    if fill == "edge":
        idx = (np.arange(nq) + rotate) % ne
        return cp.edge_q[idx].copy(), {int(p): int(i) for p, i in enumerate(idx)}
    xq = cp.plain_q[np.arange(nq) % len(cp.plain_q)].copy()
    lanes = sorted({32 * b for b in range((nq + 31) // 32)} | {min(32 * b + 31, nq - 1) for b in range((nq + 31) // 32)})
    pos = {}
    for t, lane in enumerate(lanes[:ne]):
        i = (rotate + t) % ne
        xq[lane] = cp.edge_q[i]
        pos[lane] = i
    if zero:
        assert len(cp.extra_q) and nq > 2
        xq[1] = cp.extra_q[0]
    return xq, pos


# ---- the constructions --------------------------------------------------------------------------------------------
def _ladder(kinds, seed_blocks=(140, 400), rungs=range(len(RUNGS)), turn=0):
    """two pairs per rung: four edge queries per rung, their rows rotating through the 32 positions of their blocks"""
    pairs = []
    rungs = list(rungs)
    for t in range(2 * len(rungs)):
        kind = kinds[t % len(kinds)]
        bp, bm = seed_blocks[0] + 23 * t, seed_blocks[1] + 21 * t
        pairs.append((kind, rungs[t % len(rungs)], (bp, (7 * t + 3 + turn) % BLOCK), (bm, (11 * t + 20 + turn) % BLOCK)))
    return pairs


def _hetero_pairs(kind):
    """Edge rows in blocks whose f_b is 4 x smaller (level 5) resp. 4 x larger (level 1) than both neighbours' (level 3).
    X_b is an integer norm and does not follow f_b: the neighbours of the small blocks hold a row of norm 1403 (X_b 8.6 x
    the B blocks', 2.6 x the E blocks'), the large blocks' planted rows have 4 x the norm of their neighbours' rows.
    At 20011 rows every chunk of every launch is ONE 128-row stage (plan(): rows_per_chunk = 128): the blocks below sit at
    the first and last units of chunks, behind the bootstrap and in the last rows; stage and pair boundaries INSIDE a
    chunk are hetero_wide's."""
    last_full, partial = N_ROWS // BLOCK - 1, N_ROWS // BLOCK
    small = [((128, 0), (620, 13)),                  # the first block behind the bootstrap
             ((147, 31), (156, 0)),                  # last unit of the chunk that ends at row 4736, first unit of the one at 4992
             ((199, 30), (216, 1)),                  # the same at rows 6400 and 6912
             ((383, 17), (448, 6)),                  # the same at rows 12288 and 14336
             ((partial, N_ROWS % BLOCK - 1), (310, 22))]   # row n - 1 of the partial last block
    large = [((131, 9), (last_full, 27)),            # near the first block; the last full block (its neighbour: the partial one)
             ((163, 29), (172, 2)),                  # last / first units of the chunks that meet at rows 5248 and 5504
             ((231, 31), (248, 0)),                  # at rows 7424 and 7936
             ((255, 12), (512, 25))]                 # at rows 8192 and 16384
    pairs, levels = [], {}
    for t, (sp, sm) in enumerate(small):
        pairs.append((kind, 4 - t % 2, sp, sm))
        levels[sp[0]] = levels[sm[0]] = 5
    for t, (sp, sm) in enumerate(large):
        pairs.append((kind, 4 - t % 2, sp, sm))
        levels[sp[0]] = levels[sm[0]] = 1
    return pairs, levels, [b for sp, sm in small for b, _ in (sp, sm) if b != partial]


WIDE_BATCHES = (128, 513)     # the two launch geometries hetero_wide is laid out for (one / two query blocks per wave)


def _hetero_wide_pairs():
    """200011 rows: the last slab of a search of <= 256 queries is cut into chunks of 384 rows (3 stages: pair 0 = units 0..7,
    pair 1 = units 8..11), that of 513 queries into chunks of 512 rows (two whole pairs) -- plan().  For EACH of the two
    layouts, a level-5 and a level-1 block (4 x smaller / larger f_b than both neighbours) at: unit 3 | unit 4 (the two
    sides of the stage boundary inside pair 0), unit 7 | unit 8 (the two sides of the pair boundary: other block constants
    of the same 64-byte load | the first of the NEXT load), the chunk's last unit | unit 0 of another chunk.  Every such
    block has a chunk of its own.  Returns (pairs, levels, fat, {block: (layout, unit)})."""
    pairs, levels, fat, where = [], {}, [], {}
    t = 0
    for li, nq in enumerate(WIDE_BATCHES):
        r0, r1, rpc = plan(N_WIDE, nq, 10)[-1]
        units = rpc // BLOCK
        assert rpc >= 384 and (r1 - r0) // rpc > 80
        chunk = 5 + li                                   # (the two layouts' blocks stay apart: different chunk numbers)
        for level in (5, 1):
            for ul, ur in ((3, 4), (7, 8), (units - 1, 0)):
                slots = []
                for u in (ul, ur):
                    b = (r0 + chunk * rpc) // BLOCK + u
                    chunk += 7
                    assert b not in levels and b - 1 not in levels and b + 1 not in levels
                    levels[b] = level
                    where[b] = (nq, u)
                    slots.append((b, (5 * t + 2 * li) % BLOCK))
                    if level == 5:
                        fat.append(b)
                    t += 1
                pairs.append(("E", 4 - (t // 2) % 2, slots[0], slots[1]))
    return pairs, levels, fat, where


def _make(name):
    if name == "hetero_wide":
        pairs, levels, fat, where = _hetero_wide_pairs()
        cp = build(name, pairs, levels=levels, fat=fat, a={"E": 48}, n_rows=N_WIDE, seed=19)
        cp.where = where
        return cp
    if name == "b_edge":
        # decoys: forced at 0.9 and 0.99 of the bound; 1.008 lies inside the kernel's inflation (1.6 % here); 1.05 outside
        return build(name, _ladder(("B",)), decoys=(0.9, 0.99, 1.008, 1.05), seed=11)
    if name == "e_edge":
        return build(name, _ladder(("E",), turn=1), seed=12)
    if name == "front":
        # a shard to stand in front of another corpus: E rows on Hadamard patterns the other corpora do not use
        return build(name, _ladder(("E",), turn=3), h0=4, seed=18)
    if name == "both":
        return build(name, _ladder(("BE",), turn=2), seed=13)
    if name in ("hetero", "hetero_e"):
        # (E rows with a = 48: 2.6 x below the norm of their neighbours' largest rows, 4 x above the background's)
        pairs, levels, fat = _hetero_pairs("B" if name == "hetero" else "E")
        return build(name, pairs, levels=levels, fat=fat, a={"E": 48}, seed=14)
    if name == "dim_scales":
        return build(name, _ladder(("B",), turn=4), c_exp=np.arange(DIM) % 4, seed=15)
    if name == "shifted":
        # q.mean = 2 * 127 * 16 = 4064 against scores within +-T, T ~ 2.4 * 127 / 128 * 127: more than ten times their spread
        # (the queries' weight on the two shifted dimensions, where no row has a residual, keeps a B row below
        # sqrt(125 / 127) = 0.992 of the bound: the ladder ends at the 0.97 rung)
        return build(name, _ladder(("B",), rungs=range(4), turn=5), default_level=0, a={"B": 2}, quiet={125: 16.0, 126: -16.0}, seed=16)
    if name == "const_zero":
        return build(name, _ladder(("E",), turn=6), const_dims=(5, 40, 77, 100, 101, 102, 103), zero_query=True, seed=17)
    raise KeyError(name)


# corpora whose batches are padded with their own edge queries, not with plain ones: at level 0 with a = 2 (what the 24 bits
# leave beside q.mean = 4064) the background's integer scores are smaller than the margin R grants ANY query, so a plain
# query rightly nominates every row and its merge overflows
EDGE_FILLED = ("shifted",)
NAMES = ("b_edge", "e_edge", "both", "hetero", "hetero_e", "dim_scales", "shifted", "const_zero")
COUNTED = ("b_edge", "e_edge", "hetero", "hetero_e")     # the corpora of the two-sided count check
_cache = {}


def corpus(name):
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]
