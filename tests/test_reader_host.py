"""Host side of the reader's --do_predict against the reference's own outputs (tests/golden/reader_golden.json, written by
make_reader_golden.py): pair building, answer texts, the EM metric and the alpha sweep, bit for bit.  No GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

from reader_oracle import brute_span

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "reader_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tokenizer(tmp_path_factory):
    from transformers import BertTokenizer
    d = tmp_path_factory.mktemp("vocab")
    with open(os.path.join(GOLDEN, "vocab_small.txt")) as f, open(d / "vocab.txt", "w") as g:
        g.write(f.read())
    return BertTokenizer.from_pretrained(str(d))


def test_pair_building_matches_reference(golden, tokenizer):
    from proqa_amd import qa_utils as qu
    wp = qu.WordPieces(tokenizer, threads=2)
    recs = golden["pairs"]
    prepared = qu.prepare_many([r["passage"] for r in recs], wp)
    cls_id, sep_id = tokenizer.convert_tokens_to_ids("[CLS]"), tokenizer.convert_tokens_to_ids("[SEP]")
    assert any(not r["doc_tokens"] for r in recs) and any(len(r["input_ids"]) == r["max_seq_length"] for r in recs)
    for r, p in zip(recs, prepared):
        assert p["doc_tokens"] == r["doc_tokens"]
        assert p["tok_to_orig_index"] == r["tok_to_orig_index"]
        assert p["all_doc_tokens"] == r["all_doc_tokens"]
        q_ids = tokenizer.encode(r["question"], max_length=12, truncation=True)
        assert q_ids == r["q_ids"]
        ids, seg, po, _ = qu.build_pair(q_ids, p["piece_ids"], r["max_seq_length"], cls_id, sep_id)
        assert (ids, seg, po) == (r["input_ids"], r["segment_ids"], r["para_offset"])
        mask = [1 if po <= t < len(ids) - 1 else 0 for t in range(len(ids))]
        assert mask == r["paragraph_mask"]


def test_python_fallback_of_word_pieces_matches_native(golden, tokenizer):
    from proqa_amd import qa_utils as qu
    words = [w for r in golden["pairs"] for w in r["doc_tokens"]] + ["a" * 70, "x[y]", "😀ok"]
    native = qu.WordPieces(tokenizer, threads=2)
    pieces, ids = native(words)
    for w, p, i in zip(words, pieces, ids):
        assert p == tokenizer.tokenize(w), w
        assert i == tokenizer.convert_tokens_to_ids(p)


def _sweep_from_golden(golden_predict, regex, save_prefix=None):
    from proqa_amd import qa_utils as qu
    qid2results, qid2ground = {}, {}
    for inp in golden_predict["inputs"]:
        b = inp["batch"]
        for k, qid in enumerate(b["id"]):
            n = len(b["wp_tokens"][k])
            po = b["para_offset"][k]
            s, e = np.asarray(inp["start_logits"][k], np.float32), np.asarray(inp["end_logits"][k], np.float32)
            bi, bj, bs = brute_span(s, e, po, po + n + 1)
            text = qu.answer_text(bi, bj, po, b["doc_tokens"][k], b["wp_tokens"][k], b["tok_to_orig_index"][k])
            qid2results.setdefault(qid, []).append({"text": text, "rank_score": inp["rank_logits"][k],
                                                    "span_score": float(bs) if bi >= 0 else None,
                                                    "passage": " ".join(b["doc_tokens"][k]), "question": b["q"][k]})
            qid2ground[qid] = b["true_answers"][k]
    lines = []
    _, best = qu.alpha_sweep(qid2results, qid2ground, regex=regex, save_prefix=save_prefix, out=lines.append)
    return lines, best


@pytest.mark.parametrize("regex", [False, True])
def test_alpha_sweep_matches_reference_predict(golden, tmp_path, regex):
    run = [r for r in golden["predict"]["runs"] if r["regex"] == regex][0]
    lines, best = _sweep_from_golden(golden["predict"], regex, save_prefix=str(tmp_path / "pred"))
    assert lines == run["lines"]
    assert best == run["best"]
    assert lines[0].startswith("evaluated 4 examples")       # five questions, one of them twice
    for alpha, records in run["preds"].items():
        with open(tmp_path / f"pred_{alpha}.json") as f:
            got = [json.loads(line) for line in f]
        assert got == records, alpha


def test_predict_golden_discriminates(golden, monkeypatch):
    """The golden must tell a right sweep from a wrong one: EM varies over the alphas, regex and exact differ, a tie at
    alpha 0.5 is decided by the previous alpha's order, and a broken metric does not reproduce it."""
    from proqa_amd import qa_utils as qu
    runs = {r["regex"]: r for r in golden["predict"]["runs"]}
    ems = {k: [float(l.split("EM: ")[1]) for l in r["lines"] if "EM: " in l] for k, r in runs.items()}
    assert len(set(ems[False])) >= 3 and len(set(ems[True])) >= 2 and ems[False] != ems[True]
    hamlet = [x for x in runs[False]["preds"]["0.5"] if x["question"] == "who wrote hamlet"][0]
    assert hamlet["answer"] == "Paris"           # in-place order kept at the tie; a fresh sort would pick the right answer
    monkeypatch.setattr(qu, "exact_match_score", lambda p, g: False)
    lines, _ = _sweep_from_golden(golden["predict"], False)
    assert lines != runs[False]["lines"]


def test_passage_without_span_ranks_last_at_every_alpha(tmp_path):
    """A passage without any paragraph token (span_score None, answer "") never displaces a real answer: at alpha 0 a
    -inf span score would give a NaN key and scramble the whole group's order."""
    from proqa_amd import qa_utils as qu
    group = [{"text": "a", "rank_score": 1.0, "span_score": 5.0, "passage": "A", "question": "q"},
             {"text": "", "rank_score": 0.5, "span_score": None, "passage": "", "question": "q"},
             {"text": "b", "rank_score": 3.0, "span_score": 1.0, "passage": "B", "question": "q"},
             {"text": "", "rank_score": 9.0, "span_score": None, "passage": "", "question": "q"}]
    lines = []
    qid2results = {"q": list(group)}
    res, _ = qu.alpha_sweep(qid2results, {"q": ["b"]}, save_prefix=str(tmp_path / "p"), out=lines.append)
    assert res[0] == (0, 1.0)                     # alpha 0: the best rank among the real spans, "b"
    assert res[-1] == (1, 0.0)                    # alpha 1: the best span, "a"
    with open(tmp_path / "p_0.json") as f:
        assert json.loads(f.readline())["answer"] == "b"
    assert [x["text"] for x in qid2results["q"]][-2:] == ["", ""]


def test_metric_and_text_helpers():
    from proqa_amd import qa_utils as qu
    assert qu.normalize_answer("The  Eiffel-Tower, an icon!") == "eiffeltower icon"
    assert qu.exact_match_score("the Paris", "paris")
    assert qu.regex_match_score("Paris France", r"paris")
    assert not qu.regex_match_score("x", "(")
    assert qu.metric_max_over_ground_truths(qu.exact_match_score, "1969", ["1968", "1969"])
    assert qu.hash_question("who?") == hashlib.md5("who?".encode()).hexdigest()
    assert qu.get_final_text("paris", "Paris,") == "Paris"
    assert qu.get_final_text("cafe", "café") == "café"
    assert qu.get_final_text("nowhere", "Paris") == "Paris"
    assert qu.split_words("a　b\tc  d e") == ["a", "b", "c", "d", "e"]
    assert qu.answer_text(-1, -1, 3, ["x"], ["x"], [0]) == ""


def test_training_flags_are_refused():
    from proqa_amd import predict_qa
    with pytest.raises(SystemExit, match="--do_train is not supported"):
        predict_qa.main(["--do_train"])
    with pytest.raises(SystemExit, match="only --do_predict"):
        predict_qa.main([])
