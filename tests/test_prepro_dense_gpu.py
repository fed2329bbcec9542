"""text_prefilter on the MI355X against eval_retrieval._may_match, bit for bit, and the matched-paragraph command with the
device pre-filter against the same command with the host pre-filter, byte for byte."""
import json
import os

import numpy as np
import pytest

from proqa_amd import eval_retrieval as ev

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1279, 1280, 5000]
T = b"XYZW"                                   # planted across 16- and 1024-byte boundaries
MB = "σé中x".encode()       # 2 + 3 + 3 + 1 bytes: cut at every byte by a lane boundary
T255 = bytes(65 + (i * 7) % 26 for i in range(255))
HEAD, TAIL = b"N0X", b"Z9"
ROW_END, ROW_START = b"<<E", b"B>>"
SHAPES = [(1, 1), (3, 31), (3, 32), (5, 33), (33, 70), (20, 336)]   # the last: every row is a candidate of every question


def _background(rng, n):
    return bytes(rng.choice(np.frombuffer(b"abcd e", np.uint8), size=n).tolist())


def _plant(text, at, needle):
    assert 0 <= at and at + len(needle) <= len(text)
    return text[:at] + needle + text[at + len(needle):]


def _rows(rng):
    rows = []
    for rep in range(3):                                   # every length: plain, needle at byte 0, needle ending at the end
        for n in LENGTHS:
            t = _background(rng, n)
            if rep == 1 and n >= len(HEAD):
                t = _plant(t, 0, HEAD)
            if rep == 2 and n >= len(TAIL):
                t = _plant(t, n - len(TAIL), TAIL)
            rows.append(t)
    for b in range(1, 80):                                 # T across every 16-byte boundary of a 1280-byte row, cut 1|3, 2|2, 3|1
        rows.append(_plant(_background(rng, 1280), 16 * b - 1 - b % 3, T))
    for b in range(1, 80, 2):                              # the multi-byte token, cut after each of its first 8 bytes
        rows.append(_plant(_background(rng, 1279), 16 * b - 1 - b // 2 % 8, MB))
    for m in range(1, 5):                                  # across every 1024-byte boundary of a 5000-byte row
        rows.append(_plant(_background(rng, 5000), 1024 * m - 2, T))
        rows.append(_plant(_background(rng, 5000), 1024 * m - 1 - 60 * m, T255))   # the longest token across a step
        rows.append(_plant(_plant(_background(rng, 5000), 1024 * m - 254, T255[:254]), 1024 * m, b"#"))   # all but its last byte
    rows.append(_plant(_background(rng, 5000), 5000 - 255, T255))                  # ... ending at the last byte
    rows.append(T255)                                                              # a token equal to the row
    rows.append(T255[:254])                                                        # a token longer than the row
    rows += [b"EQUALROW", b"EQUALRO", b"aaab", b"aab", b"aa", b"ab" * 40 + b"aaab", MB, MB[:-1], HEAD, TAIL, b"Z"]
    # neighbours in the blob: a needle made of the end of one row and the start of the next must not hit
    for n in (16, 64, 1024, 1280, 17, 5):
        rows.append(_plant(_background(rng, n), n - len(ROW_END), ROW_END))
        rows.append(_plant(_background(rng, 30), 0, ROW_START))
    rows.append(_plant(_background(rng, 100), 40, ROW_END + ROW_START))            # ... and inside one row it does
    while len(rows) < 300:
        rows.append(_background(rng, int(rng.integers(0, 1400))))
    return rows


def _questions(rng, rows):
    pool = [bytes([a, b]) for a in b"abcd eXYZW0N" for b in b"abcd eXYZW0N"][:128]
    qs = [
        [[T]], [[MB]], [[T255]], [[b"aab"]],
        [[HEAD, b"~~~"]],                                  # one token present, one absent
        [[b"~~~"], []],                                    # an alias without tokens: every row
        [],                                                # no alias: no row
        [[HEAD]], [[TAIL]], [[ROW_END + ROW_START]], [[b"EQUALROW"]], [[b"EQUALROWS"]],
        [[T, HEAD], [TAIL, MB]], [[T, T, HEAD]],
        [[pool[2 * i], pool[2 * i + 1]] for i in range(64)],   # 128 distinct tokens, 64 aliases
        [[b"a"]], [[b"\xcc"]], [[b" "]], [[T255[1:], T255[:-1]]], [[b"Z"], [b"9"]],
    ]
    while len(qs) < 33:                                    # tokens cut out of rows, and random ones
        aliases = []
        for _ in range(int(rng.integers(1, 4))):
            alias = []
            for _ in range(int(rng.integers(1, 4))):
                r = rows[int(rng.integers(0, len(rows)))]
                if len(r) > 8 and rng.random() < 0.7:
                    a = int(rng.integers(0, len(r) - 6))
                    alias.append(r[a:a + int(rng.integers(3, 7))])
                else:
                    alias.append(_background(rng, int(rng.integers(1, 5))))
            aliases.append(alias)
        qs.append(aliases)
    return qs


@pytest.fixture(scope="module")
def world(gpu_device):
    from proqa_amd import textstore
    rng = np.random.default_rng(2024)
    rows = _rows(rng)
    assert len(rows) == 300 and set(LENGTHS) <= {len(r) for r in rows}
    # the host blob: rows back to back behind a one-byte lead, so most start at odd offsets and neighbours touch
    blob, spans, pos = b"!", [], 1
    for r in rows:
        spans.append((pos, pos + len(r)))
        blob += r
        pos += len(r)
    assert sum(lo % 2 for lo, _ in spans) > 100
    spans = np.asarray(spans, np.int64)
    spans[7] = spans[6 + len(LENGTHS)]                     # two rows that share a text
    rows[7] = rows[6 + len(LENGTHS)]
    store = textstore.TextStore(blob, spans)
    questions = _questions(rng, rows)
    assert all(textstore.within_limits(q) for q in questions)
    # candidates [33, 336]: 36 slots of random rows, repeats, empty slots and ids outside the store, then every row once,
    # shuffled per question
    ids = np.stack([np.concatenate([rng.integers(0, 300, 31), [-1, 2 ** 40, -7, 301, 0], rng.permutation(300)])
                    for _ in range(33)]).astype(np.int64)
    ids[:, 5] = ids[:, 2]                                  # a repeat among the first slots of the small shapes
    ids[:, 9] = -1
    ids[:, 11] = 300
    for q in range(33):                                    # rows that matter to the question, early enough for k = 31
        hits = [i for i, r in enumerate(rows) if ev._may_match(questions[q], r)]
        if hits:
            ids[q, 0], ids[q, 30] = hits[0], hits[-1]
    want = np.zeros(ids.shape, bool)
    for q in range(33):
        verdict = [ev._may_match(questions[q], r) for r in rows]
        for j, i in enumerate(ids[q]):
            want[q, j] = 0 <= i < 300 and verdict[int(i)]
    yield dict(store=store, rows=rows, questions=questions, ids=ids, want=want, device=gpu_device)
    store.close()


def _bits(mask, k):
    words = mask.cpu().numpy().view(np.uint32)
    return ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(len(words), -1).astype(bool), words


def _prefilter(world, nq, k, ids=None):
    import torch
    from proqa_amd import textstore
    ids = world["ids"][:nq, :k] if ids is None else ids
    table = textstore.NeedleTable(world["questions"][:nq])
    mask, count = world["store"].prefilter(torch.from_numpy(np.ascontiguousarray(ids)).to(world["device"]), table)
    torch.cuda.synchronize()
    table.close()
    return mask, count


@pytest.mark.parametrize("nq,k", SHAPES)
def test_kernel_is_may_match_bit_for_bit(world, nq, k):
    mask, count = _prefilter(world, nq, k)
    assert tuple(mask.shape) == (nq, (k + 31) // 32)
    bits, _ = _bits(mask, k)
    assert not bits[:, k:].any(), "bits at or past k must be zero"
    want = world["want"][:nq, :k]
    wrong = np.argwhere(bits[:, :k] != want)
    assert len(wrong) == 0, [(int(q), int(j), int(world["ids"][q, j]), bool(want[q, j])) for q, j in wrong[:10]]
    np.testing.assert_array_equal(count.cpu().numpy(), want.sum(1))
    if (nq, k) == SHAPES[-1]:       # the planted cases are really there, on both sides
        rows, ids = world["rows"], world["ids"]
        hit_rows = [set(ids[q, :k][want[q]].tolist()) for q in range(nq)]
        assert len(hit_rows[0]) >= 79 + 4 and len(hit_rows[1]) >= 40 + 1 and len(hit_rows[2]) == 4 + 1 + 1
        assert want[5].sum() == ((ids[5, :k] >= 0) & (ids[5, :k] < 300)).sum() > 300 and len(hit_rows[5]) == 300
        assert not hit_rows[6] and not hit_rows[4] and not hit_rows[11]
        assert hit_rows[9] == {i for i, r in enumerate(rows) if ROW_END + ROW_START in r} and len(hit_rows[9]) == 1
        assert hit_rows[10] == {rows.index(b"EQUALROW")}
        assert hit_rows[3] >= {rows.index(b"aaab"), rows.index(b"aab"), rows.index(b"ab" * 40 + b"aaab")}
        assert rows.index(b"aa") not in hit_rows[3] and len(hit_rows[14]) > 100


def test_two_runs_agree_and_a_permutation_only_permutes(world):
    nq, k = 33, 70
    a, ca = _prefilter(world, nq, k)
    b, cb = _prefilter(world, nq, k)
    assert (a.cpu().numpy() == b.cpu().numpy()).all() and (ca.cpu().numpy() == cb.cpu().numpy()).all()
    rng = np.random.default_rng(9)
    perm = np.stack([rng.permutation(k) for _ in range(nq)])
    ids = np.take_along_axis(world["ids"][:nq, :k], perm, axis=1)
    c, cc = _prefilter(world, nq, k, ids)
    bits_a, _ = _bits(a, k)
    bits_c, _ = _bits(c, k)
    np.testing.assert_array_equal(bits_c[:, :k], np.take_along_axis(bits_a[:, :k], perm, axis=1))
    np.testing.assert_array_equal(cc.cpu().numpy(), ca.cpu().numpy())


WORDS = ("paris france capital river seine washington president united states album singer city york film tokyo japan quick "
         "brown fox lazy dog café zürich straße orwell einstein street texas neil tab ΟΔΟΣ İstanbul").split()


def test_device_route_writes_the_host_routes_file(gpu_device, tmp_path, monkeypatch):
    from proqa_amd import gen_index_id_map as gm
    from proqa_amd import npy
    from proqa_amd import prepro_dense as pd
    rng = np.random.default_rng(31)
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(0, 40)))).capitalize() + "." for _ in range(300)]
    texts[17] = texts[3]
    corpus = tmp_path / "paras.txt"
    corpus.write_text("".join(json.dumps({"id": f"p{i}", "text": t}) + "\n" for i, t in enumerate(texts)))
    gm.build(str(corpus), str(tmp_path / "idx_id.json"), texts=True)
    answers = [["Paris"], ["lazy dog", "quick brown fox"], ["zebra"], ["ΟΔΟΣ"], ["istanbul", "Zürich straße"],
               ["washington president"], ["", "never"], ["café"],
               [" ".join(f"w{i}" for i in range(130)), "tokyo japan"]]          # 130 distinct tokens: the host route
    raw = tmp_path / "qa.txt"
    raw.write_text("".join(json.dumps({"question": f"q{i}", "answer": a}) + "\n" for i, a in enumerate(answers)))
    npy.save(str(tmp_path / "para_embed.npy"), rng.standard_normal((300, 128)).astype(np.float16))
    npy.save(str(tmp_path / "query.npy"), rng.standard_normal((9, 128)).astype(np.float16))
    stats = {}
    # --num-workers 0: a test process that holds the device forks slowly (45 s for this test inside the whole suite against
    # 1 s alone); the pool itself runs in tests/test_prepro_dense_host.py
    for route in ("device", "host"):
        monkeypatch.setenv("PROQA_STATS_JSON", str(tmp_path / f"{route}.json"))
        pd.main(["--raw-data", str(raw), "--index-path", str(tmp_path / "para_embed.npy"), "--query-embed", str(tmp_path / "query.npy"),
                 "--index2paraid", str(tmp_path / "idx_id.json"), "--text-sidecar", str(tmp_path / "idx_id.txt"),
                 "--save-path", str(tmp_path / f"{route}.txt"), "--topk", "64", "--prefilter", route, "--num-workers", "0"])
        stats[route] = json.load(open(tmp_path / f"{route}.json"))
    assert (tmp_path / "device.txt").read_bytes() == (tmp_path / "host.txt").read_bytes()
    lines = [json.loads(line) for line in (tmp_path / "device.txt").read_text().splitlines()]
    assert [r["question"] for r in lines] == [f"q{i}" for i in range(9)]
    assert len(lines[0]["matched_paras"]) > 0 and lines[2]["matched_paras"] == {} and len(lines[6]["matched_paras"]) == 64
    d, h = stats["device"], stats["host"]
    assert d["host_route_questions"] == 1 and h["host_route_questions"] == 9
    for st in (d, h):
        assert st["candidates"] == 9 * 64 and st["candidates"] >= st["survivors"] >= st["confirmed"] > 0
    assert d["survivors"] == h["survivors"] and d["confirmed"] == h["confirmed"] == sum(len(r["matched_paras"]) for r in lines)
    for key in ("fold_seconds", "upload_seconds", "search_seconds", "prefilter_seconds", "confirm_seconds", "write_seconds"):
        assert d[key] >= 0
