"""NumPy float64 oracle of proqa_inbatch_eval_f16 (include/proqa_hip.h): scores from the fp16 inputs, the argmax with the
lowest-index rule, the rank of the gold column, log-sum-exp, and torch's order for non-finite scores.

Order: a NaN is greater than every number and equal to another NaN; among equal scores the lowest column wins the
argmax; a column equal to the gold beats it only from the left (j < target).  A row with a NaN has max = lse = NaN.
lse is torch.logsumexp's: the maximum is subtracted unless it is infinite, so a row with +inf gives +inf and a row of
-inf gives -inf."""
import numpy as np


def scores(q, c):
    """float64 [nq, nc] dot products of the (fp16) rows.  A product of two fp16 values is exact in float64 and 128 of
    them sum with an error below 2^-45 of their magnitudes: exact for every purpose here.  Non-finite inputs follow
    IEEE (inf * 0 = NaN, inf - inf = NaN), as the device's fp32 accumulation does."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(q, np.float64) @ np.asarray(c, np.float64).T


def abs_scores(q, c):
    """sum_d |q_d c_d|: the scale of the fp32 accumulation bound 128 * 2^-24 * sum_d |q_d c_d|."""
    return np.abs(np.asarray(q, np.float64)) @ np.abs(np.asarray(c, np.float64)).T


def accumulation_bound(q, c):
    """|fp32-accumulated score - exact score| <= 128 * 2^-24 * sum_d |q_d c_d| for ANY summation order of the 128 exact
    products (each partial sum rounds once, relative 2^-24, and is at most the absolute sum: (1 + u)^127 - 1 < 128 u)."""
    return 128.0 * 2.0 ** -24 * abs_scores(q, c)


def _greater(a, b):
    """a > b in torch's order (NaN greatest)."""
    an, bn = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        return np.where(an, ~bn, np.where(bn, False, a > b))


def _equal(a, b):
    an, bn = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        return np.where(an | bn, an & bn, a == b)


def argmax_lowest(s):
    """Lowest column among the greatest scores; the first NaN if the row has one (torch.argmax on the CPU)."""
    s = np.asarray(s)
    out = np.empty(s.shape[0], np.int32)
    for i, row in enumerate(s):
        nan = np.flatnonzero(np.isnan(row))
        out[i] = nan[0] if len(nan) else int(np.flatnonzero(row == row.max())[0])
    return out


def rank_of_gold(s, target):
    """#{j: s_ij > gold} + #{j < target_i: s_ij == gold}, in torch's order."""
    s = np.asarray(s)
    target = np.asarray(target)
    gold = s[np.arange(s.shape[0]), target][:, None]
    cols = np.arange(s.shape[1])[None, :]
    beats = _greater(s, gold) | (_equal(s, gold) & (cols < target[:, None]))
    return beats.sum(1).astype(np.int32)


def logsumexp(s):
    s = np.asarray(s, np.float64)
    out = np.empty(s.shape[0], np.float64)
    for i, row in enumerate(s):
        if np.isnan(row).any():
            out[i] = np.nan
            continue
        m = row.max()
        shift = 0.0 if np.isinf(m) else m
        with np.errstate(over="ignore", divide="ignore"):
            out[i] = np.log(np.exp(row - shift).sum()) + shift
    return out


def inbatch_eval(q, c, target=None):
    """dict(scores, argmax, rank, max, gold, lse) in float64 / int32; target None means arange(nq)."""
    s = scores(q, c)
    nq = s.shape[0]
    target = np.arange(nq) if target is None else np.asarray(target, np.int64)
    mx = np.where(np.isnan(s).any(1), np.nan, np.where(np.isnan(s), -np.inf, s).max(1)) if s.shape[1] else np.empty(0)
    return {"scores": s, "argmax": argmax_lowest(s), "rank": rank_of_gold(s, target), "max": mx,
            "gold": s[np.arange(nq), target], "lse": logsumexp(s), "target": target}


def predict_accounting(batches):
    """The reference's predict over [(q, c), ...]: (num_total as the float it prints, accuracy, per-batch argmax).  The
    reference's num_correct is a float32 tensor, so its accuracy is the float32 quotient."""
    num_total, num_correct, argmaxes = 0.0, 0.0, []
    for q, c in batches:
        a = argmax_lowest(scores(q, c))
        argmaxes.append(a)
        num_total += len(a)
        num_correct += int((a == np.arange(len(a))).sum())
    return num_total, float(np.float32(num_correct) / np.float32(num_total)), argmaxes
