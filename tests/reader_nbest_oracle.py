"""NumPy restatements of the reader's n-best span search, its log-partitions and marginal answer decoding (helpers, not
tests).  Nothing here is shared with proqa_amd: the candidates are enumerated, sorted by Python's tuple order, and the
probabilities are summed in plain float64."""
import math
import re
import string

import numpy as np


def _score_key(v):
    """-0 and +0 are one score"""
    return 0.0 if v == 0 else float(v)


def brute_nbest(start_logits, end_logits, para_offset, length, max_answer_len, n_best):
    """One sequence's (fp16) logits -> (starts, ends, scores) of n_best entries: every candidate (i, j) with
    para_offset <= i <= j < length - 1, j - i <= max_answer_len and a score fp32(start[i]) + fp32(end[j]) that is neither
    -inf nor NaN, sorted by score descending, start ascending, end ascending; (-1, -1, -inf) where there are fewer."""
    s = np.asarray(start_logits, np.float32)
    e = np.asarray(end_logits, np.float32)
    cands = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(max(para_offset, 0), length - 1):
            for j in range(i, min(i + max_answer_len, length - 2) + 1):
                v = np.float32(s[i] + e[j])
                if v > -np.inf:         # false for NaN too
                    cands.append((-_score_key(v), i, j, v))
    cands.sort(key=lambda c: c[:3])
    starts = np.full(n_best, -1, np.int32)
    ends = np.full(n_best, -1, np.int32)
    scores = np.full(n_best, -np.inf, np.float32)
    for n, (_, i, j, v) in enumerate(cands[:n_best]):
        starts[n], ends[n], scores[n] = i, j, v
    return starts, ends, scores


def lse64(x):
    """float64 log-sum-exp of the values x: -inf when empty or all -inf, +inf when one is +inf (and none NaN)"""
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return -np.inf
    if np.isnan(x).any():
        return np.nan
    m = float(x.max())
    if math.isinf(m):
        return m
    return m + math.log(float(np.exp(x - m).sum()))


def lse32_sequential(x):
    """the same in float32, one term after the other: max, then sum += exp(x - max) in row order, then max + log(sum);
    exp and log are correctly rounded (taken in float64, rounded to float32), so the figure does not depend on a vector
    library's last bit"""
    x = np.asarray(x, np.float32)
    if x.size == 0:
        return np.float32(-np.inf)
    m = np.float32(x.max())
    if np.isinf(m):
        return m
    acc = np.float32(0)
    for v in x:
        acc = np.float32(acc + np.float32(math.exp(float(np.float32(v - m)))))
    return np.float32(m + np.float32(math.log(float(acc))))


def paragraph_lse(start_logits, end_logits, para_offset, length, fn=lse64):
    """(Z^s, Z^e) of one sequence: fn over the paragraph rows [para_offset, length - 1)"""
    par = slice(max(para_offset, 0), max(length - 1, 0))
    return fn(np.asarray(start_logits)[par]), fn(np.asarray(end_logits)[par])


def lse_error(got, ref):
    """max|got - ref| / max|ref| over the finite entries of ref (0 when there is none); the others must be equal"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (got[~fin], ref[~fin])
    if not fin.any():
        return 0.0
    return float(np.abs(got[fin] - ref[fin]).max() / max(np.abs(ref[fin]).max(), 1e-30))


# ---- marginal decoding -----------------------------------------------------------------------------------------------

def _normalize_answer(s):
    s = "".join(ch for ch in s.lower() if ch not in set(string.punctuation))
    s = re.sub(r"\b(a|an|the)\b", " ", s)
    return " ".join(s.split())


def _lse_list(xs):
    xs = [float(x) for x in xs]
    m = max(xs)
    if math.isinf(m):
        return m
    return m + math.log(sum(math.exp(x - m) for x in xs))


def marginal(results, norm):
    """results: [dict(rank_score, lse = (Z^s, Z^e), candidates = [(text, score)])] of one question, in retrieval order
    -> [(key, P, text of the first mention)] by P descending, ties to the first mention.
    P(key) = sum over mentions of exp(score - Z + log r_b); log r = log-softmax of the rank scores; Z = Z^s_b + Z^e_b
    ("passage") or logsumexp_b Z^s_b + logsumexp_b Z^e_b ("shared").  Empty texts only count when nothing else exists."""
    assert norm in ("shared", "passage")
    if not results:
        return []
    zr = _lse_list([x["rank_score"] for x in results])
    z_shared = _lse_list([x["lse"][0] for x in results]) + _lse_list([x["lse"][1] for x in results])
    mentions = []
    for x in results:
        z = z_shared if norm == "shared" else float(x["lse"][0]) + float(x["lse"][1])
        for text, score in x["candidates"]:
            l = float(score) - z + float(x["rank_score"]) - zr
            if not math.isnan(l):
                mentions.append((text, l))
    if any(t.strip() for t, _ in mentions):
        mentions = [(t, l) for t, l in mentions if t.strip()]
    table = {}          # key -> [P, text, position of the first mention]
    for pos, (text, l) in enumerate(mentions):
        row = table.setdefault(_normalize_answer(text), [0.0, text, pos])
        row[0] += math.exp(l) if l < 700 else math.inf
    return [(k, v[0], v[1]) for k, v in sorted(table.items(), key=lambda kv: (-kv[1][0], kv[1][2]))]
