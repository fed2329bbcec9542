"""The int8 quantiser of the k <= 128 search and its nomination bound, restated in NumPy -- TEST INFRASTRUCTURE ONLY (CPU).

What proqa_amd/csrc/mips_kernels.hip defines at the top of its "int8 nomination scan" section (column_stats_finish,
quantise_rows_i8, prep_queries_i8, lane_threshold / block_threshold), for one shard of fp16 rows:

    per shard   mean_d, c_d = max |x_d - mean_d| (a constant dimension: c = 0, quantises to 0)
    per block   f_b = max |u| over the 32 rows (u = (x - mean) / c), G_b = 127 / f_b, xi = clamp(rint(127 u / f_b)),
                r = 127 u / f_b - xi, X_b = max ||xi||; rows past n in the last block count as the mean
    per shard   R = max ||r||, Xf = max ||x||
    per query   w = q c, s_q = max |w| / 127, qi = clamp(rint(w / s_q)), e = w / s_q - qi, ||w / s_q||, ||e||, q.mean

The numbers that DECIDE something -- mean, c, f_b, xi, s_q, qi -- are computed as the kernels compute them, in float32 with
the same operations in the same order (the mean is float32(sum / n) of a float64 sum: the kernel's float32 partial sums
are exact on the grids the edge corpora live on, and on other rows nothing depends on the mean's accuracy).  Everything
MEASURED against them -- the residuals r and e, their norms, q.mean, the shortfall and the bound -- is float64 on the fp16
inputs, relative to those float32 values taken as exact reals, so that the identity

    q.x - q.mean = (f_b / 127) s_q [acc + sum_d e_d xi_d + sum_d (w_d / s_q) r_d],      acc = qi.xi

holds to float64 rounding and |shortfall| <= bound is Cauchy-Schwarz and nothing else.  (s_q here is 1 / inv_unit, the
reciprocal the kernel multiplies by, not the quotient max |w| / 127 it was made from.)"""
import numpy as np

DIM = 128
BLOCK = 32
_F = np.float32


class Rows:
    """quantise_rows_i8 on one shard"""

    def __init__(self, xb):
        xb = np.asarray(xb)
        assert xb.dtype == np.float16 and xb.ndim == 2 and xb.shape[1] == DIM
        n = xb.shape[0]
        self.n = n
        x64 = xb.astype(np.float64)
        x32 = xb.astype(_F)
        # column_stats_finish
        mean = (x64.sum(axis=0) / float(n)).astype(_F)
        c = np.maximum(x32.max(axis=0) - mean, mean - x32.min(axis=0)).astype(_F)
        with np.errstate(divide="ignore"):
            inv_c = np.where(c > 0, _F(1) / c, _F(0)).astype(_F)
        self.mean, self.c = mean.astype(np.float64), c.astype(np.float64)
        # quantise_rows_i8 (rows past n: u = 0)
        nb = (n + BLOCK - 1) // BLOCK
        u32 = np.zeros((nb * BLOCK, DIM), _F)
        u32[:n] = (x32 - mean) * inv_c
        f = np.abs(u32).reshape(nb, BLOCK * DIM).max(axis=1).astype(_F)
        f[~(f > 0)] = _F(1)
        G32 = (_F(127) / f).astype(_F)
        t32 = u32 * np.repeat(G32, BLOCK)[:, None]
        xi = np.clip(np.rint(t32), -127, 127)
        self.xi = xi[:n].astype(np.int32)
        self.f = f.astype(np.float64)
        self.G = 127.0 / self.f                                   # the exact real; the kernel's float32 G_b is within 2^-24 of it
        self.block_of_row = np.arange(n) // BLOCK
        # measured against those: u as a real number, r = 127 u / f_b - xi
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(self.c > 0, (x64 - self.mean) / self.c, 0.0)
        self.r = u * self.G[self.block_of_row][:, None] - self.xi
        xin = np.zeros(nb * BLOCK)
        xin[:n] = np.sqrt((self.xi.astype(np.float64) ** 2).sum(axis=1))
        self.X = xin.reshape(nb, BLOCK).max(axis=1)
        self.R = float(np.sqrt((self.r ** 2).sum(axis=1)).max())
        self.Xf = float(np.sqrt((x64 ** 2).sum(axis=1)).max())
        self.x64 = x64


class Queries:
    """prep_queries_i8 on a batch, against the shard statistics of `rows`"""

    def __init__(self, xq, rows):
        xq = np.asarray(xq)
        assert xq.dtype == np.float16 and xq.ndim == 2 and xq.shape[1] == DIM
        q64 = xq.astype(np.float64)
        w32 = xq.astype(_F) * rows.c.astype(_F)
        wmax = np.abs(w32).max(axis=1).astype(_F)
        s32 = (wmax / _F(127)).astype(_F)
        ok = (s32 > 0) & np.isfinite(s32)
        with np.errstate(divide="ignore"):
            inv32 = np.where(ok, _F(1) / np.where(ok, s32, _F(1)), _F(0)).astype(_F)
        self.qi = np.clip(np.rint(w32 * inv32[:, None]), -127, 127).astype(np.int32)
        self.inv = inv32.astype(np.float64)                        # inv_unit = 1 / s_q (0 for a zero query)
        w = q64 * rows.c                                           # exact: an fp16 times a float32 fits a float64
        self.wn = w * self.inv[:, None]                            # w / s_q
        self.e = self.wn - self.qi
        self.n_u = np.sqrt((self.wn ** 2).sum(axis=1))
        self.n_e = np.sqrt((self.e ** 2).sum(axis=1))
        self.n_q = np.sqrt((q64 ** 2).sum(axis=1))
        self.off = q64 @ rows.mean                                 # q.mean
        self.abs_off = np.abs(q64 * rows.mean).sum(axis=1)
        self.q64 = q64


class Oracle:
    def __init__(self, xb, xq):
        self.rows = Rows(xb)
        self.queries = Queries(xq, self.rows)
        self._acc = None
        self._scores = None

    # ---- the four quantities of the derivation, for all (query, row) pairs at once: arrays [nq, n] / [nq, blocks] ----
    def acc(self):
        """the exact integer score qi.xi (|acc| <= 127 * 127 * 128 < 2^53: the float64 product is exact)"""
        if self._acc is None:
            self._acc = self.queries.qi.astype(np.float64) @ self.rows.xi.astype(np.float64).T
        return self._acc

    def scores(self):
        """q.x in float64 (exact on the edge corpora: every partial sum fits 24 bits there)"""
        if self._scores is None:
            self._scores = self.queries.q64 @ self.rows.x64.T
        return self._scores

    def units(self):
        """[nq, n]: integer units per score unit of (query, row's block), G_b / s_q"""
        return self.queries.inv[:, None] * self.rows.G[self.rows.block_of_row][None, :]

    def shortfall(self):
        """[q.x - q.mean] / ((f_b / 127) s_q) - acc, in integer units (0 for a zero query)"""
        return (self.scores() - self.queries.off[:, None]) * self.units() - self.acc()

    def bound(self):
        """[nq, blocks]: ||w / s_q|| R + ||e|| X_b"""
        q, r = self.queries, self.rows
        return q.n_u[:, None] * r.R + q.n_e[:, None] * r.X[None, :]

    def row_bound(self):
        return self.bound()[:, self.rows.block_of_row]

    # ---- the two sets of the count check ----
    def true_threshold(self, tau):
        """[nq, n]: A G_b - B - E X_b as real numbers, no inflation: a row whose exact score beats tau lies above it"""
        q = self.queries
        A = (np.asarray(tau, np.float64) - q.off) * q.inv
        return A[:, None] * self.rows.G[self.rows.block_of_row][None, :] - self.row_bound()

    def forced(self, tau):
        """[nq, n] bool: the pairs the real inequality acc > A G_b - B - E X_b forces a sound scan to nominate"""
        return self.acc() > self.true_threshold(tau)

    def kernel_threshold(self, tau):
        """[nq, n]: the kernel's own documented formula in float64 -- prep_queries_i8's off, delta, margin_r and err_norm with
        their (1 + 2^-10) factors and the + 2^-6, quantise_rows_i8's rounded-up R, Xf and X_b, lane_threshold's 2^-20"""
        q, r = self.queries, self.rows
        up = 1.0 + 2.0 ** -10
        R = r.R * up + 2.0 ** -10
        Xf = r.Xf * up
        n_u, n_e, n_q = q.n_u * up, q.n_e * up + 2.0 ** -10, q.n_q * up
        off32 = q.off.astype(_F).astype(np.float64)
        delta = 2.0 ** -14 * n_q * Xf + 2.0 ** -20 * q.abs_off
        off = off32 + delta + np.abs(off32) * 2.0 ** -22
        margin_r = n_u * R * up + 2.0 ** -6
        a = (np.asarray(tau, np.float64) - off) * q.inv
        A = a - np.abs(a) * 2.0 ** -20
        Xb = (r.X * up)[r.block_of_row]
        return A[:, None] * r.G[r.block_of_row][None, :] - margin_r[:, None] - n_e[:, None] * Xb[None, :]

    def allowed(self, tau):
        """[nq, n] bool: the pairs above the kernel's formula, lowered by one further integer unit for the float32 rounding
        of the threshold (two fused multiply-adds on values below 2^21: far less than one unit)"""
        return self.acc() > self.kernel_threshold(tau) - 1.0


def lowest_bit_exponent(x):
    """exponent of the lowest set bit of each (finite, float64-held) value; a large number for zeros"""
    m, e = np.frexp(np.asarray(x, np.float64))
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    tz = np.where(mi != 0, np.log2(np.maximum(low, 1).astype(np.float64)).astype(np.int64), 0)
    return np.where(mi != 0, e.astype(np.int64) - 53 + tz, 1 << 20)


def partial_sums_fit_24_bits(xq, xb, chunk=2048):
    """True iff for every (query, row) the products q_d x_d are all multiples of one power of two g with
    sum_d |q_d x_d| < 2^24 g: every partial sum of the dot product, in any order, is then an exact float32."""
    q64, x64 = np.asarray(xq, np.float64), np.asarray(xb, np.float64)
    lq, lx = lowest_bit_exponent(q64), lowest_bit_exponent(x64)
    aq = np.abs(q64)
    worst = -np.inf
    for r0 in range(0, len(x64), chunk):
        ax, lxc = np.abs(x64[r0:r0 + chunk]), lx[r0:r0 + chunk]
        mag = aq @ ax.T                                            # [nq, rows]
        # first the grid every product certainly lies on (finest bit of the query + finest bit of the row); the exact one --
        # a (min, +) product over the dimensions -- only for the rows where that is not enough
        g = np.minimum(lq.min(axis=1)[:, None] + lxc.min(axis=1)[None, :], 1 << 20)
        with np.errstate(divide="ignore"):
            hard = np.flatnonzero(((mag > 0) & (np.log2(mag) - g >= 24.0)).any(axis=0))
        if len(hard):
            gh = np.full((len(aq), len(hard)), 1 << 20, np.int64)
            for d in range(x64.shape[1]):
                np.minimum(gh, lq[:, d][:, None] + lxc[hard, d][None, :], out=gh)
            g[:, hard] = gh
        live = mag > 0
        if live.any():
            worst = max(worst, float((np.log2(mag[live]) - g[live]).max()))
    return worst < 24.0, worst
