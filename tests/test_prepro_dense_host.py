"""The matched-paragraph file (proqa_amd.prepro_dense) and the host side of the device pre-filter (proqa_amd.textstore):
folding, the reference's outputs (matched_golden.json, made by the reference's own process_qa_para over recall_docs.db), the
superset property the pre-filter rests on, and what the entry points refuse before they touch a device."""
import ctypes
import json
import os

import numpy as np
import pytest

from proqa_amd import _lib
from proqa_amd import eval_retrieval as ev
from proqa_amd import prepro_dense as pd
from proqa_amd import textstore as ts
from proqa_amd.utils import normalize

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DB = os.path.join(GOLDEN, "recall_docs.db")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "matched_golden.json")) as f:
        g = json.load(f)
    ev.init(DB)
    return g


def test_fold_is_the_scorers_fold_in_utf8():
    cases = ["", "Paris", "İstanbul İ", "ΟΔΟΣ Σσς ς", "Beyoncé é É",
             "Zürich STRASSE Straße", "東京 Tōkyō", "á̧ ṩ", "tab\tnew\nline", "Σ", "O'Neil's 3.5-star"]
    for t in cases:
        want = ev._fold(normalize(t)).encode()
        assert ts.TextStore.fold(t) == want and ts.fold(t) == want, t
    assert ts.TextStore.fold("") == b""
    assert ts.TextStore.fold("İ") == "i̇".encode()            # one character lower-cases to two
    assert ts.TextStore.fold("Σς") == "σσ".encode()      # both sigmas are one
    assert ts.TextStore.fold("é") == ts.TextStore.fold("é") == b"e\xcc\x81"   # NFD


def _run(tmp_path, case, match, capsys, workers=2, **kw):
    raw = tmp_path / f"raw_{match}.txt"
    ret = tmp_path / f"retrieved_{match}.txt"
    out = tmp_path / f"matched_{match}.txt"
    raw.write_text("".join(json.dumps(q) + "\n" for q in case["raw"]))
    ret.write_text("".join(json.dumps(r) + "\n" for r in case["retrieved"]))
    capsys.readouterr()
    assert pd.process_ground_paras(str(ret), str(out), str(raw), workers, False, case["k"], match, prefilter="host", **kw) is None
    printed = capsys.readouterr().out.strip().splitlines()
    return [json.loads(line) for line in out.read_text().splitlines()], printed


def _sidecar(tmp_path):
    from proqa_amd import gen_index_id_map as gm
    with open(os.path.join(GOLDEN, "recall_golden.json")) as f:
        docs = json.load(f)["docs"]
    corpus = tmp_path / "paras.txt"
    corpus.write_text("".join(json.dumps({"id": d[0], "text": d[1]}) + "\n" for d in docs))
    gm.build(str(corpus), str(tmp_path / "idx_id.json"), texts=True)
    return str(tmp_path / "idx_id.json"), str(tmp_path / "idx_id.txt")


@pytest.mark.parametrize("texts", ["db", "sidecar", "sidecar, no pool"])
def test_string_mode_reproduces_the_reference(gold, tmp_path, capsys, texts):
    case = gold["string"]
    kw = {"db_path": DB}
    if texts != "db":
        idx, txt = _sidecar(tmp_path)
        kw = {"index2paraid": idx, "text_sidecar": txt, "workers": 2 if texts == "sidecar" else 0}
    state = (ev.PROCESS_TOK, ev.PROCESS_DB, ev.PROCESS_TEXTS)
    lines, printed = _run(tmp_path, case, "string", capsys, **kw)
    assert (ev.PROCESS_TOK, ev.PROCESS_DB, ev.PROCESS_TEXTS) == state      # (num_workers 0 works in this process)
    assert printed[-1] == case["coverage"]                       # the reference's print(np.mean(topk_covered))
    assert len(lines) == len(case["lines"])
    for got, want in zip(lines, case["lines"]):                  # input order; keys in candidate order; matched strings
        assert got == want
        assert list(got["matched_paras"].items()) == list(want["matched_paras"].items())
        assert list(got) == list(want)
    st = pd.LAST_RUN_STATS
    assert st["candidates"] >= st["survivors"] >= st["confirmed"] == sum(len(w["matched_paras"]) for w in case["lines"])
    assert st["candidates"] == sum(min(len(r["para_id"]), case["k"]) for r in case["retrieved"])
    assert st["survivors"] < st["candidates"]                   # the pre-filter rejects something


def test_regex_mode_reproduces_the_reference(gold, tmp_path, capsys):
    case = gold["regex"]
    lines, printed = _run(tmp_path, case, "regex", capsys, db_path=DB)
    assert printed[-1] == case["coverage"]
    assert lines[3]["matched_paras"] == {}                      # the pattern that does not compile matches nothing
    assert len(lines) == len(case["lines"])
    for got, want in zip(lines, case["lines"]):
        assert list(got) == list(want)
        assert list(got["matched_paras"]) == list(want["matched_paras"])
        assert got == want      # de-duplicated and sorted (the reference's set order is arbitrary: the golden file sorts it)
    assert pd.LAST_RUN_STATS["prefilter"] == "none" and pd.LAST_RUN_STATS["host_route_questions"] == 0


def test_stats_file_and_unknown_ids(gold, tmp_path, capsys, monkeypatch):
    case = gold["string"]
    idx, txt = _sidecar(tmp_path)
    monkeypatch.setenv("PROQA_STATS_JSON", str(tmp_path / "stats.json"))
    _run(tmp_path, case, "string", capsys, index2paraid=idx, text_sidecar=txt)
    st = json.load(open(tmp_path / "stats.json"))
    for key in ("search_seconds", "prefilter_seconds", "confirm_seconds", "write_seconds", "candidates", "survivors",
                "confirmed", "host_route_questions"):
        assert key in st, key
    bad = dict(case, retrieved=[dict(r) for r in case["retrieved"]])
    bad["retrieved"][2] = {"para_id": ["d1", "no-such-id"]}
    with pytest.raises(ValueError, match="no-such-id"):
        _run(tmp_path, bad, "string", capsys, index2paraid=idx, text_sidecar=txt)
    with pytest.raises(ValueError, match="text_sidecar"):        # the device route reads texts by row
        pd.process_ground_paras(None, str(tmp_path / "o"), str(tmp_path / "raw_string.txt"), 2, index_path="x", query_embeds="y",
                                index2paraid=str(tmp_path / "missing.json"))


def _reference_match(answer, para):
    """the reference's loop (qa/prepro_dense.py:44-55): tokenise everything, compare runs of words"""
    text = ev.PROCESS_TOK.tokenize(normalize(para)).words(uncased=True)
    for alias in answer:
        needle = ev.PROCESS_TOK.tokenize(normalize(alias)).words(uncased=True)
        for i in range(len(text) - len(needle) + 1):
            if text[i:i + len(needle)] == needle:
                return True
    return False


def test_an_exact_match_implies_a_prefilter_hit_on_the_folded_bytes(gold):
    """What the device sees is bytes: folded UTF-8 needles inside the folded UTF-8 passage.  Over 10 000 random (answer,
    paragraph) pairs of the adversarial alphabet (both sigmas, the dotted capital I, combining marks, apostrophes, CJK, empty
    and punctuation-only aliases) every pair the reference matches passes the byte test, and the byte test is the scorer's
    character test."""
    rng = np.random.default_rng(17)
    alphabet = list("abAB ΣσςΟΔİéé'.-中") + ["  "]

    def rand_text(n):
        return "".join(rng.choice(alphabet, size=n))

    matched = passed = 0
    for _ in range(10000):
        para = rand_text(int(rng.integers(0, 48)))
        answer = [rand_text(int(rng.integers(0, 6))) for _ in range(int(rng.integers(1, 4)))]
        if rng.random() < 0.3 and len(para) > 4:
            a = int(rng.integers(0, len(para) - 2))
            answer.append(para[a:a + int(rng.integers(1, 7))].swapcase())
        needles = [ev._words(alias) for alias in answer]
        folded = ts.fold_needles(needles)
        hit = ev._may_match(folded, ts.fold(para))                                   # bytes in bytes
        assert hit == ev._may_match([[ev._fold(t) for t in n] for n in needles], ev._fold(normalize(para))), (answer, para)
        want = _reference_match(answer, para)
        assert hit or not want, (answer, para)
        matched += want
        passed += hit
    assert 500 < matched <= passed < 9500


def _needles_rc(questions):
    lib = _lib.load()
    arrays = ts.pack_needles(questions)
    h = ctypes.c_void_p()
    rc = lib.proqa_text_needles_create(*[a.ctypes.data for a in arrays], len(questions), ctypes.byref(h))
    assert not h.value or rc == 0
    if h.value:
        lib.proqa_text_needles_destroy(h)
    return rc, lib.proqa_last_error().decode()


def test_entry_points_refuse_over_limit_input_before_touching_a_device():
    lib = _lib.load()
    ok = [[[b"a"]]]
    for questions, words in [
        (ok + [[[b"x" * 256]]], "256 bytes"),                                           # token length
        (ok + [[[b"%03d" % i for i in range(129)]]], "129 distinct tokens"),            # tokens per question
        (ok + [[[b"a"]] * 65], "65 aliases"),                                           # aliases per question
        (ok + [[[bytes([65 + i]) * 200 for i in range(21)]]], "4200 needle bytes"),     # needle bytes per question
    ]:
        assert not ts.within_limits(questions[-1])
        rc, msg = _needles_rc(questions)
        assert rc == -1 and words in msg and "question 1" in msg, msg
    assert ts.within_limits([[b"x" * 255], []]) and ts.within_limits([[b"%03d" % i for i in range(128)]] * 64)
    h = ctypes.c_void_p()
    # an empty token, and an alias that names a token its question does not have
    tb, toff, qt, at, aoff, qa = ts.pack_needles([[[b"ab", b"c"]]])
    toff2 = np.asarray([0, 2, 2], np.int64)
    assert lib.proqa_text_needles_create(tb.ctypes.data, toff2.ctypes.data, qt.ctypes.data, at.ctypes.data, aoff.ctypes.data,
                                         qa.ctypes.data, 1, ctypes.byref(h)) == -1
    at2 = np.asarray([0, 2], np.int32)
    assert lib.proqa_text_needles_create(tb.ctypes.data, toff.ctypes.data, qt.ctypes.data, at2.ctypes.data, aoff.ctypes.data,
                                         qa.ctypes.data, 1, ctypes.byref(h)) == -1
    assert b"alias token index 2" in lib.proqa_last_error()
    assert lib.proqa_text_needles_create(None, None, None, None, None, None, -1, ctypes.byref(h)) == -1
    # the pre-filter call itself: k, nq, NULL handles
    assert lib.proqa_text_prefilter(None, None, None, 1, 16385, None, None, None) == -1 and b"k 16385" in lib.proqa_last_error()
    assert lib.proqa_text_prefilter(None, None, None, 1, 0, None, None, None) == -1
    assert lib.proqa_text_prefilter(None, None, None, -1, 8, None, None, None) == -1 and b"negative nq" in lib.proqa_last_error()
    assert lib.proqa_text_prefilter(None, None, None, 1, 8, None, None, None) == -1 and b"NULL store" in lib.proqa_last_error()
    # the store: spans outside the blob, negative sizes
    blob = np.frombuffer(b"abcdef", np.uint8)
    for spans in ([[0, 7]], [[4, 2]], [[-1, 3]]):
        s = np.asarray(spans, np.int64)
        assert lib.proqa_textstore_create(blob.ctypes.data, 6, s.ctypes.data, 1, ctypes.byref(h)) == -1
        assert b"outside the blob" in lib.proqa_last_error() and not h.value
    assert lib.proqa_textstore_create(blob.ctypes.data, -1, None, 0, ctypes.byref(h)) == -1
    assert lib.proqa_textstore_destroy(None) == 0 and lib.proqa_text_needles_destroy(None) == 0
    assert lib.proqa_textstore_info(None, None, None) == -1


def test_fold_sidecar_shares_repeated_texts(tmp_path):
    from proqa_amd import gen_index_id_map as gm
    texts = ["İstanbul", "", "Paris", "İstanbul", "Σς", "Paris", ""]
    gm.write_text_sidecar(texts, str(tmp_path / "t"))
    for workers in (0, 2):
        blob, spans, seconds = ts.fold_sidecar(str(tmp_path / "t.txt"), workers=workers, chunk=2)
        assert [bytes(blob[lo:hi]) for lo, hi in spans] == [ts.fold(t) for t in texts] and seconds >= 0
        assert tuple(spans[0]) == tuple(spans[3]) and tuple(spans[2]) == tuple(spans[5])
        assert len(blob) == sum(len(ts.fold(t)) for t in set(texts))


def test_command_line_names_the_missing_input(tmp_path):
    raw = tmp_path / "raw.txt"
    raw.write_text("")
    with pytest.raises(SystemExit, match="--raw-data"):
        pd.main([])
    with pytest.raises(SystemExit, match="--save-path"):
        pd.main(["--raw-data", str(raw)])
    base = ["--raw-data", str(raw), "--save-path", str(tmp_path / "out.txt")]
    with pytest.raises(SystemExit, match="--index-path"):
        pd.main(base)
    with pytest.raises(SystemExit, match="--query-embed"):
        pd.main(base + ["--index-path", str(raw)])
    with pytest.raises(SystemExit, match="--index2paraid"):
        pd.main(base + ["--index-path", str(raw), "--query-embed", str(raw)])
    with pytest.raises(SystemExit, match="--text-sidecar"):
        pd.main(base + ["--index-path", str(raw), "--query-embed", str(raw), "--index2paraid", str(raw)])
    with pytest.raises(SystemExit, match="--query-embed: no such file"):
        pd.main(base + ["--index-path", str(raw), "--query-embed", str(tmp_path / "nope.npy"), "--index2paraid", str(raw),
                        "--text-sidecar", str(raw)])
    with pytest.raises(SystemExit):
        pd.main(base + ["--match", "fuzzy"])
    a = pd.build_parser().parse_args(base)
    assert (a.topk, a.match, a.prefilter, a.num_workers) == (10000, "string", "device", 40)
