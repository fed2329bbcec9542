"""Seeded inputs of the reader's online-sampler golden (shared by tests/golden/make_reader_sampler_golden.py and the tests).

A corpus of N_ROWS passages over the words of tests/golden/vocab_small.txt, one 128-d row per passage and one vector per
question with entries m/8, |m| <= 8 (every inner product is a multiple of 1/64 below 2^7: exact in float32, and the rows
and vectors are exact in fp16, so the order of the retrieval is decided by the tie rule alone: descending score, ties
to the ascending row).  The retrieval is computed HERE first, and the texts of the retrieved passages and the gold lists
are then written around it, so that the cases the golden must contain exist by construction:

    question 0   no gold row in its top 5000 and no answer in its top K passages             -> {}
    question 1   no gold row at all, one of the top K passages carries the answer
    question 2   gold rows in the top 5000, no answer in the top K passages
    question 3   a 60-word passage whose answer lies past the cut of max_length
    question 4   a passage with the answer three times (and once glued to punctuation), others with one or none:
                 start / end rows padded with -1 beside real positions
    question 5   two answers, one of one word and one of two; both cases of a letter -> two matched strings
    question 6   a question longer than max_query_length; a gold id that names no row of the index, one outside the
                 top 5000, and the first and the last id of the top 5000
    question 7   a regex-like plain answer that occurs nowhere; gold rows only                -> labels only
"""
import json
import os
import sqlite3

import numpy as np

N_ROWS = 5200
K_SEARCH = 5000
K = 5
MAX_LENGTH = 48
MAX_QUERY_LENGTH = 12
SEED = 20240611

# never drawn as filler: the answers are made of these
RESERVED = ("paris", "france", "queen", "king", "new", "york", "river", "album", "band", "university")

QUESTIONS = [
    ("where was the first president born", ["university band"]),
    ("what is the capital city of france", ["paris"]),
    ("who was the queen", ["queen"]),
    ("which river", ["river album"]),
    ("what state is the school in", ["new york"]),
    ("who was he", ["king", "new york"]),
    ("when was the first film of the united states team in the world war season game", ["france"]),
    ("what was it", ["album of the king"]),
]


def vocab_words(vocab_path):
    words = [l.rstrip("\n") for l in open(vocab_path, encoding="utf-8")]
    plain = [w for w in words if w.isalnum() and not w.startswith("[") and w not in RESERVED and len(w) > 1]
    suffixes = [w[2:] for w in words if w.startswith("##") and w[2:].isalpha()]
    return plain, suffixes


def para_id(row):
    return f"p{row * 7 + 3}"


def _filler(rng, plain, suffixes, n):
    out = []
    for _ in range(n):
        w = plain[int(rng.integers(len(plain)))]
        r = int(rng.integers(12))
        if r == 0 and suffixes:
            w = w + suffixes[int(rng.integers(len(suffixes)))]      # more than one piece
        elif r == 1:
            w = w.capitalize()
        elif r == 2:
            w = w + ","
        out.append(w)
    return out


def _plant(words, at, text):
    """words with `text` (one or more words) put in place of the words from position `at` on"""
    new = text.split()
    return words[:at] + new + words[at + len(new):]


def make_inputs(vocab_path):
    """-> dict(rows fp16 [N,128], q_vectors fp32 [8,128], passages [N] str, index2paraid {str(row): id},
    questions [{"question", "answer"}], matched [{"question", "matched_paras": {para id: str}}], top [8, K_SEARCH] rows)"""
    rng = np.random.default_rng(SEED)
    plain, suffixes = vocab_words(vocab_path)
    rows = (rng.integers(-8, 9, (N_ROWS, 128)) / 8.0).astype(np.float16)
    qv = (rng.integers(-8, 9, (len(QUESTIONS), 128)) / 8.0).astype(np.float32)
    rows[100] = rows[50]                     # exact ties: equal rows ...
    rows[4000] = rows[50]
    scores = qv.astype(np.float64) @ rows.astype(np.float64).T
    top = np.argsort(-scores, axis=1, kind="stable")[:, :K_SEARCH]
    head = top[:, :K]
    assert len(set(head.reshape(-1).tolist())) == head.size, "the top-K rows of the questions must be distinct"

    passages = [" ".join(_filler(rng, plain, suffixes, int(rng.integers(8, 61)))) for _ in range(N_ROWS)]

    def rewrite(row, n_words, plants):
        words = _filler(rng, plain, suffixes, n_words)
        for at, text in plants:
            words = _plant(words, at, text)
        passages[row] = " ".join(words)

    gold = [dict() for _ in QUESTIONS]
    outside = [sorted(set(range(N_ROWS)) - set(top[q].tolist())) for q in range(len(QUESTIONS))]

    # 0: gold rows only outside the top 5000; nothing planted
    for r in outside[0][:3]:
        gold[0][para_id(r)] = "university band"
    # 1: no gold; the third passage carries the answer, glued to a comma
    rewrite(int(head[1, 2]), 20, [(7, "Paris,")])
    # 2: gold rows inside the top 5000 (not among the top K), nothing planted
    for r in top[2, [5, 77, 4999]].tolist():
        gold[2][para_id(r)] = "queen"
    # 3: the answer at words 55-56 of a 60-word passage (max_length 48 cuts before it); one gold row
    rewrite(int(head[3, 0]), 60, [(55, "river album")])
    rewrite(int(head[3, 4]), 9, [(2, "river album")])
    gold[3][para_id(int(head[3, 0]))] = "river album"
    gold[3][para_id(int(top[3, 1234]))] = "river album"
    # 4: three occurrences in one passage (one in brackets), one in another, none in the rest
    rewrite(int(head[4, 1]), 30, [(1, "new york"), (9, "(New York)"), (20, "new york")])
    rewrite(int(head[4, 3]), 12, [(10, "new york")])
    gold[4][para_id(int(head[4, 1]))] = "new york"
    gold[4][para_id(int(head[4, 3]))] = "new york"
    # 5: two answers; "King" and "king" are two matched strings of one passage
    rewrite(int(head[5, 0]), 25, [(0, "King"), (5, "new york"), (11, "king")])
    rewrite(int(head[5, 2]), 8, [(7, "king")])
    gold[5][para_id(int(head[5, 0]))] = "King"
    # 6: long question; gold ids: no row of the index, outside the top 5000, the first and the last of the top 5000
    rewrite(int(head[6, 4]), 40, [(17, "France")])
    gold[6]["p-not-in-the-index"] = "france"
    gold[6][para_id(outside[6][0])] = "france"
    gold[6][para_id(int(top[6, 0]))] = "france"
    gold[6][para_id(int(top[6, 4999]))] = "france"
    # 7: gold rows only
    for r in top[7, [0, 1, 2, 3, 4, 2500]].tolist():
        gold[7][para_id(r)] = "album of the king"

    index2paraid = {str(r): para_id(r) for r in range(N_ROWS)}
    questions = [{"question": q, "answer": a} for q, a in QUESTIONS]
    matched = [{"question": q, "matched_paras": gold[i]} for i, (q, _) in enumerate(QUESTIONS)]
    return {"rows": rows, "q_vectors": qv, "passages": passages, "index2paraid": index2paraid, "questions": questions,
            "matched": matched, "top": top}


def write_files(inputs, tmp):
    """raw data, matched file, idx_id.json, sqlite DB and the rows' .npy under `tmp` -> dict of paths"""
    paths = {n: os.path.join(tmp, f) for n, f in (("raw", "train.txt"), ("matched", "matched.txt"), ("idx", "idx_id.json"),
                                                  ("db", "paras.db"), ("npy", "para_embed.npy"))}
    with open(paths["raw"], "w") as f:
        for q in inputs["questions"]:
            f.write(json.dumps(q) + "\n")
    with open(paths["matched"], "w") as f:
        for m in inputs["matched"]:
            f.write(json.dumps(m) + "\n")
    with open(paths["idx"], "w") as f:
        json.dump(inputs["index2paraid"], f)
    con = sqlite3.connect(paths["db"])
    con.execute("CREATE TABLE documents (id PRIMARY KEY, text)")
    con.executemany("INSERT INTO documents VALUES (?, ?)",
                    [(para_id(r), p) for r, p in enumerate(inputs["passages"])])
    con.commit()
    con.close()
    np.save(paths["npy"], inputs["rows"])
    return paths
