"""Host side of the reader's online sampler against tests/golden/reader_sampler_golden.json (recorded from the reference's
OnlineSampler.load by tests/golden/make_reader_sampler_golden.py): answer matching, offsets, spans, the truncation rule and
the pair building of the top-k passages; regex matching on hand-made cases; the gold-row CSR."""
import json
import os

import numpy as np
import pytest

import reader_sampler_inputs as gen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "reader_sampler_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def inputs():
    return gen.make_inputs(os.path.join(GOLDEN, "vocab_small.txt"))


@pytest.fixture(scope="module")
def tokenizer(tmp_path_factory):
    from transformers import BertTokenizer
    d = tmp_path_factory.mktemp("vocab")
    with open(os.path.join(GOLDEN, "vocab_small.txt")) as f, open(d / "vocab.txt", "w") as g:
        g.write(f.read())
    return BertTokenizer.from_pretrained(str(d))


def test_generator_is_the_recorded_retrieval(golden, inputs):
    assert golden["k"] == gen.K and golden["max_length"] == gen.MAX_LENGTH
    assert len(golden["questions"]) == len(inputs["questions"]) == 8
    for q, rec in enumerate(golden["questions"]):
        if rec:
            assert rec["first_ids"] == inputs["top"][q, :gen.K].tolist()
            assert rec["last_id"] == int(inputs["top"][q, -1]) and rec["n_ids"] == gen.K_SEARCH


def test_spans_and_pairs_match_the_reference(golden, inputs, tokenizer):
    from proqa_amd import qa_utils as qu
    from proqa_amd.basic_tokenizer import SimpleTokenizer
    from proqa_amd.online_sampler import passage_spans, prepare_passages, span_positions
    wp = qu.WordPieces(tokenizer, threads=2)
    basic = SimpleTokenizer()
    cls_id, sep_id = tokenizer.vocab["[CLS]"], tokenizer.vocab["[SEP]"]
    seen = {"cut": 0, "multi": 0, "padded": 0, "empty": 0}
    for q, rec in enumerate(golden["questions"]):
        qa = inputs["questions"][q]
        rows = inputs["top"][q, :gen.K].tolist()
        preps = prepare_passages([qu.normalize(inputs["passages"][r]) for r in rows], wp)
        spans = [passage_spans(p, qa["answer"], basic, tokenizer.tokenize) for p in preps]
        if not rec:
            # {}: no answer in the top k (and, by the generator, no gold row in the top 5000)
            assert not any(c for c, _, _ in spans)
            seen["empty"] += 1
            continue
        q_ids = tokenizer.encode(qa["question"], max_length=gen.MAX_QUERY_LENGTH, truncation=True)
        assert [q_ids] * gen.K == rec["input_ids_q"]
        width = len(rec["start_positions"][0])
        for b, (prep, (covered, starts, ends)) in enumerate(zip(preps, spans)):
            ids, seg, po, keep = qu.build_pair(q_ids, prep["piece_ids"], gen.MAX_LENGTH, cls_id, sep_id)
            n = rec["seq_lens"][b]
            assert ids == rec["input_ids"][b][:n] and seg == rec["segment_ids"][b][:n] and len(ids) == n
            assert not any(rec["input_ids"][b][n:]) and not any(rec["segment_ids"][b][n:])
            assert po == rec["para_offset"][b] and rec["paragraph_mask_runs"][b] == [po, n - 1]
            st, en, cov = span_positions(keep, po, covered, starts, ends)
            want = sorted((s, e) for s, e in zip(rec["start_positions"][b], rec["end_positions"][b]) if s >= 0)
            got = sorted((s, e) for s, e in zip(st, en) if s >= 0)
            assert got == want, (q, b)
            assert cov == rec["para_targets"][b]
            assert all((s < 0) == (e < 0) for s, e in zip(st, en))
            seen["cut"] += int(covered and not cov)
            seen["multi"] += int(len(got) >= 2)
            seen["padded"] += int(0 < len(got) < width)
    assert all(seen.values()), seen


def test_offsets():
    from proqa_amd import qa_utils as qu
    text = "  ab  c　de "
    assert qu.split_words(text) == ["ab", "c", "de"]
    assert qu.char_to_word_offset(text) == [-1, -1, 0, 0, 0, 0, 1, 1, 2, 2, 2]
    assert qu.orig_to_tok_index([0, 0, 1, 3, 3], 4) == [0, 2, 3, 3]       # word 2 has no piece
    assert qu.orig_to_tok_index([], 0) == []


def test_improve_answer_span_prefers_the_leftmost_longest():
    from proqa_amd import qa_utils as qu
    pieces = ["(", "new", "york", ")", "new", "york"]
    assert qu._improve_answer_span(pieces, 0, 3, "new york") == (1, 2)
    assert qu._improve_answer_span(pieces, 0, 5, "new york") == (1, 2)
    assert qu._improve_answer_span(pieces, 0, 3, "paris") == (0, 3)


def test_string_matching_is_sorted_and_uncased():
    from proqa_amd import qa_utils as qu
    from proqa_amd.basic_tokenizer import SimpleTokenizer
    p = "the king , The King and the KING of New  York"
    assert qu.match_answer_span(p, ["the king", "new york"], SimpleTokenizer()) == ["New  York", "The King", "the KING", "the king"]
    assert qu.match_answer_span(p, ["queen"], SimpleTokenizer()) == []
    with pytest.raises(ValueError):
        qu.match_answer_span(p, ["queen"], SimpleTokenizer(), match="fuzzy")


def test_regex_matching():
    from proqa_amd import qa_utils as qu
    from proqa_amd.basic_tokenizer import SimpleTokenizer
    p = "Apollo 11 landed in 1969 , Apollo 12 in 1969 and skylab in 1973"
    assert qu.match_answer_span(p, [r"19[0-9]{2}", "ignored"], SimpleTokenizer(), match="regex") == ["1969", "1973"]
    assert qu.match_answer_span(p, [r"apollo \d+"], SimpleTokenizer(), match="regex") == ["Apollo 11", "Apollo 12"]   # IGNORECASE
    assert qu.match_answer_span(p, [r"^skylab"], SimpleTokenizer(), match="regex") == []
    assert qu.match_answer_span(p, [r"(unbalanced"], SimpleTokenizer(), match="regex") == []                            # does not compile


def test_regex_spans_through_the_offsets(tokenizer):
    """a regex match inside a word glued to punctuation: the pieces of the word, narrowed to the answer's"""
    from proqa_amd import qa_utils as qu
    from proqa_amd.basic_tokenizer import SimpleTokenizer
    from proqa_amd.online_sampler import passage_spans, prepare_passages
    wp = qu.WordPieces(tokenizer, threads=1)
    prep = prepare_passages(["the king of (paris), paris france"], wp)[0]
    covered, starts, ends = passage_spans(prep, [r"par[a-z]s"], SimpleTokenizer(), tokenizer.tokenize, regex=True)
    pieces = prep["all_doc_tokens"]
    assert covered == 1 and [pieces[s:e + 1] for s, e in zip(starts, ends)] == [["paris"], ["paris"]]
    assert starts == [pieces.index("paris"), len(pieces) - 2]


@pytest.mark.parametrize("form", ["dict", "list"])
def test_gold_row_csr(form):
    from proqa_amd.online_sampler import gold_row_csr, invert_index2paraid
    from proqa_amd.qa_utils import hash_question
    ids = [f"para-{r}" for r in range(10)]
    index2paraid = {str(r): p for r, p in enumerate(ids)} if form == "dict" else ids
    inv = invert_index2paraid(index2paraid)
    assert inv == {p: r for r, p in enumerate(ids)}
    matched = {hash_question("q one"): {"para-7": "x", "para-2": "x", "not-a-row": "x", "para-9": "x"},
               hash_question("q two"): {},
               hash_question("q three"): {"para-0": "x"},
               hash_question("never asked"): {"para-1": "x"}}
    rows, offsets, slots = gold_row_csr(["q one", "q two", "q one", "q three"], matched, inv)
    assert rows.dtype == np.int64 and rows.tolist() == [2, 7, 9, 0] and offsets.tolist() == [0, 3, 3, 4]
    assert slots == {hash_question("q one"): 0, hash_question("q two"): 1, hash_question("q three"): 2}
    with pytest.raises(ValueError, match="q four"):
        gold_row_csr(["q one", "q four"], matched, inv)
