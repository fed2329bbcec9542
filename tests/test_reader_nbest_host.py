"""Host side of the n-best span search and marginal answer decoding: the oracle against the existing best-span oracle,
qa_utils.marginal_answers on a question worked by hand, the command line's two flags, the entry point's refusals, and the
lse error table of test_reader_nbest_gpu.py."""
import ctypes
import math

import numpy as np
import pytest

import reader_nbest_oracle as oracle
import test_reader_nbest_gpu as G
from reader_oracle import brute_span


@pytest.mark.parametrize("seed", range(6))
def test_oracle_first_entry_is_the_existing_best_span(seed):
    """seeded logits on a coarse grid (many equal scores), some -inf; every max_answer_len"""
    rng = np.random.default_rng(seed)
    L = int(rng.integers(4, 60))
    po = int(rng.integers(0, L))
    s = (rng.integers(-4, 5, L) / 2).astype(np.float16)
    e = (rng.integers(-4, 5, L) / 2).astype(np.float16)
    if seed % 2:
        s[rng.integers(0, L, 3)] = -np.inf
        e[rng.integers(0, L, 3)] = -np.inf
    for mal in (0, 3, 10, 64):
        bi, bj, bs = brute_span(s, e, po, L, mal)
        starts, ends, scores = oracle.brute_nbest(s, e, po, L, mal, 1)
        assert (int(starts[0]), int(ends[0])) == (bi, bj), (seed, mal)
        assert np.float32(scores[0]).view(np.int32) == np.float32(bs).view(np.int32)
        # and the first entry of a longer list is the same; the list is ordered and holds no pair twice
        starts, ends, scores = oracle.brute_nbest(s, e, po, L, mal, 32)
        assert (int(starts[0]), int(ends[0])) == (bi, bj)
        k = int((starts >= 0).sum())
        keys = list(zip((-scores[:k]).tolist(), starts[:k].tolist(), ends[:k].tolist()))
        assert keys == sorted(keys) and len(set(keys)) == k
        assert (starts[k:] == -1).all() and (ends[k:] == -1).all() and np.isneginf(scores[k:]).all()


def _hand_question():
    """Three passages, equal rank scores (log r = -log 3).  Z^s = Z^e = 0 for all of them.
    passage 0: "Lyon" at score -0.5; passages 1 and 2: "Paris" / "paris." at -1.0 each, and "the Seine" at -3.0 in 1."""
    return [
        {"rank_score": 2.0, "lse": (0.0, 0.0), "candidates": [("Lyon", -0.5)]},
        {"rank_score": 2.0, "lse": (0.0, 0.0), "candidates": [("Paris", -1.0), ("the Seine", -3.0)]},
        {"rank_score": 2.0, "lse": (0.0, 0.0), "candidates": [("paris.", -1.0)]},
    ]


def test_marginal_answers_by_hand_two_moderate_mentions_beat_one_outlier():
    from proqa_amd import qa_utils as qu
    q = _hand_question()
    # the 1-best alpha rule sees one span per passage and, with equal rank scores, picks the highest span score: "Lyon"
    entries = [{"text": x["candidates"][0][0], "rank_score": x["rank_score"], "span_score": x["candidates"][0][1]} for x in q]
    for alpha in qu.ALPHAS:
        assert sorted(entries, key=qu.sweep_key(alpha), reverse=True)[0]["text"] == "Lyon"
    # passage norm: Z = 0 + 0.  P(paris) = 2 e^-1 / 3 = 0.2453, P(lyon) = e^-0.5 / 3 = 0.2022, P(seine) = e^-3 / 3
    got = qu.marginal_answers(q, "passage")
    assert [a["key"] for a in got] == ["paris", "lyon", "seine"]
    assert [a["text"] for a in got] == ["Paris", "Lyon", "the Seine"]
    np.testing.assert_allclose([a["prob"] for a in got], [2 * math.exp(-1) / 3, math.exp(-0.5) / 3, math.exp(-3) / 3],
                               rtol=1e-14)
    # shared norm: Z = log 3 + log 3, every probability 9 times smaller, the same order
    got = qu.marginal_answers(q, "shared")
    assert [a["key"] for a in got] == ["paris", "lyon", "seine"]
    np.testing.assert_allclose([a["prob"] for a in got], [2 * math.exp(-1) / 27, math.exp(-0.5) / 27, math.exp(-3) / 27],
                               rtol=1e-14)


def test_marginal_answers_norms_differ_and_can_disagree():
    """Passage 0 is flat (large Z), passage 1 peaked (small Z): the passage norm divides each by its own Z and prefers the
    peaked passage's answer, the shared norm divides both by the same Z and prefers the higher raw score.
      scores: "rome" 3.0 in passage 0 (Z^s + Z^e = 4.0), "oslo" 2.0 in passage 1 (Z^s + Z^e = 2.5), equal ranks (r = 1/2)
      passage: P(rome) = e^(3 - 4) / 2 = 0.1839, P(oslo) = e^(2 - 2.5) / 2 = 0.3033           -> oslo
      shared:  Z = 2 logsumexp(2.0, 1.25) = 2 * 2.38687 = 4.77374
               P(rome) = e^(3 - 4.77374) / 2 = 0.08485, P(oslo) = e^(2 - 4.77374) / 2 = 0.03121 -> rome"""
    from proqa_amd import qa_utils as qu
    q = [{"rank_score": 0.0, "lse": (2.0, 2.0), "candidates": [("Rome", 3.0)]},
         {"rank_score": 0.0, "lse": (1.25, 1.25), "candidates": [("Oslo", 2.0)]}]
    got = qu.marginal_answers(q, "passage")
    assert [a["key"] for a in got] == ["oslo", "rome"]
    np.testing.assert_allclose([a["prob"] for a in got], [math.exp(-0.5) / 2, math.exp(-1.0) / 2], rtol=1e-14)
    z = 2 * math.log(math.exp(2.0) + math.exp(1.25))
    assert abs(z - 4.77374) < 1e-5
    got = qu.marginal_answers(q, "shared")
    assert [a["key"] for a in got] == ["rome", "oslo"]
    np.testing.assert_allclose([a["prob"] for a in got], [math.exp(3 - z) / 2, math.exp(2 - z) / 2], rtol=1e-14)
    np.testing.assert_allclose([a["prob"] for a in got], [0.08485, 0.03121], rtol=1e-3)


def test_marginal_answers_rank_weights_ties_and_empty_texts():
    from proqa_amd import qa_utils as qu
    # rank scores log 3 and 0: r = (3/4, 1/4); the same span score: "b" of the first passage wins 3 to 1
    q = [{"rank_score": math.log(3.0), "lse": (0.0, 0.0), "candidates": [("b", 0.0)]},
         {"rank_score": 0.0, "lse": (0.0, 0.0), "candidates": [("a", 0.0)]}]
    got = qu.marginal_answers(q, "passage")
    assert [(a["key"], a["text"]) for a in got] == [("b", "b"), ("", "a")]       # normalize_answer drops the article "a"
    np.testing.assert_allclose([a["prob"] for a in got], [0.75, 0.25], rtol=1e-14)
    # equal probabilities: the first mention in (passage, n) order comes first
    q = [{"rank_score": 1.0, "lse": (0.0, 0.0), "candidates": [("y", -1.0), ("x", -1.0)]},
         {"rank_score": 1.0, "lse": (0.0, 0.0), "candidates": [("z", -1.0)]}]
    assert [a["key"] for a in qu.marginal_answers(q, "shared")] == ["y", "x", "z"]
    # empty texts are dropped ...
    q = [{"rank_score": 1.0, "lse": (0.0, 0.0), "candidates": [("", 5.0), ("x", -1.0)]},
         {"rank_score": 1.0, "lse": (-np.inf, -np.inf), "candidates": []}]
    assert [a["text"] for a in qu.marginal_answers(q, "passage")] == ["x"]
    assert [a["text"] for a in qu.marginal_answers(q, "shared")] == ["x"]
    # ... unless nothing else exists; no mention at all gives no answer
    q[0]["candidates"] = [("", 5.0)]
    assert [a["text"] for a in qu.marginal_answers(q, "passage")] == [""]
    q[0]["candidates"] = []
    assert qu.marginal_answers(q, "shared") == [] and qu.marginal_answers([], "shared") == []
    with pytest.raises(ValueError):
        qu.marginal_answers(q, "question")


@pytest.mark.parametrize("seed", range(4))
def test_marginal_answers_equals_the_oracle(seed):
    from proqa_amd import qa_utils as qu
    rng = np.random.default_rng(seed)
    words = ["Paris", "paris", "the Paris", "Lyon", "lyon!", "", "Oslo", "a", "Rome  "]
    q = []
    for b in range(int(rng.integers(1, 7))):
        n = int(rng.integers(0, 6))
        lse = (float(rng.normal(3, 1)), float(rng.normal(3, 1))) if n else (-np.inf, -np.inf)
        q.append({"rank_score": float(rng.normal(0, 2)), "lse": lse,
                  "candidates": [(str(rng.choice(words)), float(np.float32(rng.normal(2, 2)))) for _ in range(n)]})
    for norm in ("shared", "passage"):
        got, want = qu.marginal_answers(q, norm), oracle.marginal(q, norm)
        assert [(a["key"], a["text"]) for a in got] == [(k, t) for k, _, t in want]
        np.testing.assert_allclose([a["prob"] for a in got], [p for _, p, _ in want], rtol=1e-12)


def test_parser_accepts_the_flags_and_keeps_its_defaults():
    from proqa_amd import predict_qa
    p = predict_qa.build_parser()
    base = vars(p.parse_args(["--do_predict"]))
    assert base["n_best"] == 0 and base["marginal"] == "shared"
    args = vars(p.parse_args(["--do_predict", "--n-best", "20", "--marginal", "passage"]))
    assert args["n_best"] == 20 and args["marginal"] == "passage"
    assert {k: v for k, v in args.items() if k not in ("n_best", "marginal")} == \
           {k: v for k, v in base.items() if k not in ("n_best", "marginal")}
    # every earlier default is where it was
    assert base["eval_k"] == 5 and base["reader_batch"] == 256 and base["search"] == "exact" and base["prefix"] == "eval"
    assert base["max_seq_length"] == 512 and base["save_pred"] is False and base["regex"] is False
    with pytest.raises(SystemExit):
        p.parse_args(["--do_predict", "--marginal", "question"])
    for bad in (-1, 33):
        with pytest.raises(SystemExit):
            predict_qa.check_search_args(p.parse_args(["--do_predict", "--n-best", str(bad)]))
    predict_qa.check_search_args(p.parse_args(["--do_predict", "--n-best", "32"]))


def test_abi_refuses_bad_sizes_without_a_gpu():
    from proqa_amd import _lib
    lib = _lib.load()

    def call(n_best=5, mal=10, batch=4, seq_len=64, hidden=128):
        # NULL device pointers: every call below is refused before anything could be dereferenced
        return lib.proqa_reader_span_nbest_f16(None, None, None, batch, seq_len, hidden, None, None, None, mal, n_best, None,
                                               None, None, None, None, None)

    for kw in (dict(n_best=0), dict(n_best=33), dict(n_best=-1), dict(mal=-1), dict(seq_len=4097), dict(seq_len=0),
               dict(hidden=12), dict(hidden=2048), dict(batch=-1)):
        assert call(**kw) == -1, kw
    assert call(n_best=33) == -1 and b"n_best=33" in lib.proqa_last_error()
    assert call() == -1 and b"NULL" in lib.proqa_last_error()           # sizes in range: the NULL pointers are next
    assert call(batch=0, n_best=32, mal=0) == 0                          # nothing to do
    assert lib.proqa_abi_version() == 7


def test_lse_error_table_is_reproduced():
    """the GPU test's lse bounds are four times these numbers; they are measured here, on the CPU"""
    table = G.measure_reference_error()
    assert set(table) == set(G.REFERENCE_LSE_ERROR)
    for name, v in table.items():
        want = G.REFERENCE_LSE_ERROR[name]
        assert abs(v - want) <= 0.1 * want, (name, v, want)
    # the cases are what the GPU test says they are
    c = G.make_case("overflow")
    lg = G.host_logits(c).astype(np.float32)
    assert np.isposinf(lg[10]).all() and np.isneginf(lg[14]).all() and np.isneginf(lg[40 + 12]).all()
    z = G.case_lse(c, lg, oracle.lse64)
    assert np.isposinf(z[0]).all() and np.isfinite(z[1]).all()
    c = G.make_case("ties")
    lg = G.host_logits(c).astype(np.float32)
    assert (lg * 16 == np.round(lg * 16)).all()
    _, _, scores = oracle.brute_nbest(lg[:200, 0], lg[:200, 1], 5, 200, 10, 32)
    assert len(set(scores.tolist())) < 8
    z = G.case_lse(G.make_case("ragged"), G.host_logits(G.make_case("ragged")).astype(np.float32), oracle.lse64)
    assert np.isneginf(z[3]).all() and np.isfinite(np.delete(z, 3, 0)).all()
