"""proqa_reader_span_nbest_f16, BertReader.forward(n_best=...) and `--do_predict --n-best` on the GPU.

The selection is exact: starts, ends and score bits must equal tests/reader_nbest_oracle.py's enumeration over the GPU's OWN
logits_out (the logits themselves are held to the oracle by test_reader_gpu.py), entry 0 and the logits must equal
proqa_reader_span_f16's outputs bit for bit, and two runs must be bit-identical.

lse_out is compared with the float64 log-sum-exp of the GPU's logits.  Error measure: max|got - ref| / max|ref| over the
finite entries of a case (the others -- -inf for an empty paragraph, +inf beside a +inf logit -- must be equal).  Bound:
four times the same error of a float32 sequential restatement (oracle.lse32_sequential: max, sum += exp(x - max) in row
order, max + log(sum), exp and log correctly rounded), measured on the CPU by measure_reference_error() over logits formed in float64 from the same
inputs and rounded to fp16 (the host test reproduces the table):

    case        lse error
    ragged      2.558e-08
    ties        5.702e-08
    long        6.670e-08
    limit       5.184e-07
    overflow    5.216e-08
"""
import functools
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import reader_nbest_oracle as oracle

pytestmark = pytest.mark.gpu

REFERENCE_LSE_ERROR = {"ragged": 2.558e-08, "ties": 5.702e-08, "long": 6.670e-08, "limit": 5.184e-07, "overflow": 5.216e-08}

# name: lens, para_offset, H.  ragged: sequence 3 has an empty paragraph, sequence 4 one row, sequence 5 four rows
GEOMETRY = {
    "ragged": ([40, 33, 25, 12, 9, 8], [6, 9, 5, 11, 7, 3], 128),
    "ties": ([200, 77], [5, 10], 128),
    "long": ([512, 512, 500, 301], [10, 14, 9, 12], 768),
    "limit": ([4096], [17], 128),
    "overflow": ([40, 30], [5, 4], 128),
}


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict(hidden fp16 [T, H] packed, qa_w fp16 [2, H], qa_b fp16 [2], lens, para_offset)"""
    lens, po, H = GEOMETRY[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    T = sum(lens)
    if name == "ties":
        # everything a multiple of 1/8 and only four live columns: the logits are multiples of 1/16 in [-0.5, 0.5], so
        # the ~2000 candidates of a sequence share ~30 scores
        hidden = rng.integers(-8, 9, (T, H)).astype(np.float32) / 8
        hidden[:, :4] = rng.integers(-2, 3, (T, 4)).astype(np.float32) / 8
        w = np.zeros((2, H), np.float32)
        w[0, 0], w[0, 1], w[1, 2], w[1, 3] = 1.0, 0.5, 1.0, 0.5
        b = np.array([0.125, -0.125], np.float32)
    else:
        hidden = rng.standard_normal((T, H)).astype(np.float32)
        w = (0.3 * rng.standard_normal((2, H)) / np.sqrt(H / 128)).astype(np.float32)
        b = (0.1 * rng.standard_normal(2)).astype(np.float32)
    if name == "overflow":
        # positive weights: a row of 65504s gives +inf for both logits, a row of -65504s -inf for both.  Sequence 0 has
        # +inf at 10 and -inf at 14: (10, 14) is inf - inf, every (i, 10) and (10, j) else is +inf; sequence 1 only -inf
        w = np.abs(w) + 0.05
        hidden[10], hidden[14] = 65504.0, -65504.0
        hidden[lens[0] + 12] = -65504.0
    return dict(hidden=hidden.astype(np.float16), qa_w=w.astype(np.float16), qa_b=b.astype(np.float16), lens=lens,
                para_offset=po)


def host_logits(c):
    """the head's logits formed in float64 and rounded to fp16, [T, 2] (the GPU's differ in a last bit here and there)"""
    with np.errstate(over="ignore"):
        lg = c["hidden"].astype(np.float64) @ c["qa_w"].astype(np.float64).T + c["qa_b"].astype(np.float64)
        return lg.astype(np.float16)


def case_lse(c, lg, fn):
    """[B, 2] of fn over every sequence's paragraph rows of the packed logits lg"""
    row0 = np.concatenate([[0], np.cumsum(c["lens"])])
    return np.array([oracle.paragraph_lse(lg[row0[b]:row0[b + 1], 0], lg[row0[b]:row0[b + 1], 1], c["para_offset"][b],
                                          c["lens"][b], fn) for b in range(len(c["lens"]))])


def measure_reference_error():
    """{case: lse error of the float32 sequential restatement against float64}, on the CPU"""
    table = {}
    for name in GEOMETRY:
        c = make_case(name)
        lg = host_logits(c).astype(np.float32)
        table[name] = oracle.lse_error(case_lse(c, lg, oracle.lse32_sequential), case_lse(c, lg, oracle.lse64))
    return table


# ---- the kernel ------------------------------------------------------------------------------------------------------

def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def lib(gpu_device):
    from proqa_amd import _lib
    return _lib.load()


def _device_case(c, d, padded, S):
    hid = torch.from_numpy(c["hidden"]).to(d)
    if padded:
        row0 = np.concatenate([[0], np.cumsum(c["lens"])])
        pad = torch.zeros((len(c["lens"]) * S, hid.shape[1]), dtype=torch.float16, device=d)
        for b, n in enumerate(c["lens"]):
            pad[b * S:b * S + n] = hid[row0[b]:row0[b + 1]]
        hid = pad
    return hid, torch.from_numpy(c["qa_w"]).to(d), torch.from_numpy(c["qa_b"]).to(d)


def run(lib, d, c, n_best, mal=10, padded=False, S=None):
    """(nbest start, end [B, N], score [B, N], lse [B, 2], 1-best start, end, score [B], logits [T, 2] fp16 packed):
    both entry points on one case; guard rows behind every output; the two kernels' logits must be the same bits"""
    from proqa_amd import _lib
    lens, po = c["lens"], c["para_offset"]
    B, S = len(lens), S or max(lens)
    hid, qa_w, qa_b = _device_case(c, d, padded, S)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=d)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=d)
    po_t = torch.tensor(po, dtype=torch.int32, device=d)
    layout = (hid.data_ptr(), lens_t.data_ptr() if padded else None, None if padded else cu.data_ptr(), B, S, hid.shape[1],
              po_t.data_ptr(), qa_w.data_ptr(), qa_b.data_ptr(), mal)
    nb_start = torch.full((B + 1, n_best), -7, dtype=torch.int32, device=d)
    nb_end = torch.full((B + 1, n_best), -7, dtype=torch.int32, device=d)
    nb_score = torch.full((B + 1, n_best), 3.0, dtype=torch.float32, device=d)
    lse = torch.full((B + 1, 2), 3.0, dtype=torch.float32, device=d)
    logits = torch.full((hid.shape[0] + 1, 2), 3.0, dtype=torch.float16, device=d)
    _lib.check(lib.proqa_reader_span_nbest_f16(*layout, n_best, nb_start.data_ptr(), nb_end.data_ptr(), nb_score.data_ptr(),
                                               lse.data_ptr(), logits.data_ptr(), stream()))
    start = torch.full((B,), -7, dtype=torch.int32, device=d)
    end = torch.full((B,), -7, dtype=torch.int32, device=d)
    score = torch.zeros(B, dtype=torch.float32, device=d)
    logits1 = torch.full((hid.shape[0] + 1, 2), 3.0, dtype=torch.float16, device=d)
    _lib.check(lib.proqa_reader_span_f16(*layout, start.data_ptr(), end.data_ptr(), score.data_ptr(), logits1.data_ptr(),
                                         stream()))
    assert torch.equal(logits.view(torch.int16), logits1.view(torch.int16)), "the two span kernels' logits differ"
    for t in (nb_start, nb_end):
        assert (t[-1] == -7).all(), "wrote past the last row"
    assert (nb_score[-1] == 3.0).all() and (lse[-1] == 3.0).all() and (logits[-1] == 3.0).all(), "wrote past the last row"
    lg = logits[:-1].cpu().numpy()
    if padded:
        lg = np.concatenate([lg[b * S:b * S + n] for b, n in enumerate(lens)])
    return (nb_start[:-1].cpu().numpy(), nb_end[:-1].cpu().numpy(), nb_score[:-1].cpu().numpy(), lse[:-1].cpu().numpy(),
            start.cpu().numpy(), end.cpu().numpy(), score.cpu().numpy(), lg)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check(c, out, n_best, mal, lse_bound):
    nb_start, nb_end, nb_score, lse, start, end, score, lg = out
    # entry 0 is the 1-best kernel's answer
    assert (nb_start[:, 0] == start).all() and (nb_end[:, 0] == end).all() and (bits(nb_score[:, 0]) == bits(score)).all()
    lg32 = lg.astype(np.float32)
    row0 = np.concatenate([[0], np.cumsum(c["lens"])])
    for b, n in enumerate(c["lens"]):
        s, e, v = oracle.brute_nbest(lg32[row0[b]:row0[b + 1], 0], lg32[row0[b]:row0[b + 1], 1], c["para_offset"][b], n, mal,
                                     n_best)
        assert (nb_start[b] == s).all() and (nb_end[b] == e).all(), (b, nb_start[b], s, nb_end[b], e)
        assert (bits(nb_score[b]) == bits(v)).all(), (b, nb_score[b], v)
    err = oracle.lse_error(lse, case_lse(c, lg32, oracle.lse64))
    print(f"lse error {err:.3e} (bound {lse_bound:.3e})")
    assert err <= lse_bound


def same(a, b):
    return all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


def test_ragged_batch_every_n_and_length_cap(lib, gpu_device):
    c = make_case("ragged")
    for n_best in (1, 5, 20, 32):
        for mal in (0, 10, 64):
            out = run(lib, gpu_device, c, n_best, mal)
            check(c, out, n_best, mal, 4 * REFERENCE_LSE_ERROR["ragged"])
    nb_start, nb_end, nb_score, lse = out[:4]
    assert (nb_start[3] == -1).all() and (nb_end[3] == -1).all() and np.isneginf(nb_score[3]).all()    # empty paragraph
    assert np.isneginf(lse[3]).all()
    assert (nb_start[4, 0], nb_end[4, 0]) == (7, 7) and (nb_start[4, 1:] == -1).all() and np.isneginf(nb_score[4, 1:]).all()
    assert (nb_start[5, :10] >= 3).all() and (nb_start[5, 10:] == -1).all()       # four rows: 4 + 3 + 2 + 1 candidates
    assert same(out, run(lib, gpu_device, c, 32, 64)), "two runs differ"


def test_ties_resolve_by_start_then_end(lib, gpu_device):
    c = make_case("ties")
    out = run(lib, gpu_device, c, 32, 10)
    check(c, out, 32, 10, 4 * REFERENCE_LSE_ERROR["ties"])
    nb_start, nb_end, nb_score = out[:3]
    for b in range(2):      # the case is what it claims: equal scores inside the n-best, in position order
        assert len(set(nb_score[b].tolist())) < 8
        keys = list(zip((-nb_score[b]).tolist(), nb_start[b].tolist(), nb_end[b].tolist()))
        assert keys == sorted(keys)
    assert same(out, run(lib, gpu_device, c, 32, 10)), "two runs differ"


def test_long_sequences_packed_and_padded(lib, gpu_device):
    c = make_case("long")
    out = run(lib, gpu_device, c, 20, 10)
    check(c, out, 20, 10, 4 * REFERENCE_LSE_ERROR["long"])
    assert same(out, run(lib, gpu_device, c, 20, 10, padded=True, S=512)), "padded and packed layouts differ"
    assert same(out, run(lib, gpu_device, c, 20, 10)), "two runs differ"


def test_one_sequence_of_4096_rows(lib, gpu_device):
    c = make_case("limit")
    out = run(lib, gpu_device, c, 32, 10)
    check(c, out, 32, 10, 4 * REFERENCE_LSE_ERROR["limit"])
    assert same(out, run(lib, gpu_device, c, 32, 10)), "two runs differ"


def test_overflowed_logits(lib, gpu_device):
    c = make_case("overflow")
    out = run(lib, gpu_device, c, 20, 10)
    nb_start, nb_end, nb_score, lse, _, _, _, lg = out
    assert np.isposinf(lg[10].astype(np.float32)).all() and np.isneginf(lg[14].astype(np.float32)).all()
    check(c, out, 20, 10, 4 * REFERENCE_LSE_ERROR["overflow"])
    # +inf scores in position order: the starts 5 .. 9 that reach end 10, then start 10 with its ends but 14 (inf - inf)
    assert np.isposinf(nb_score[0, :15]).all() and np.isfinite(nb_score[0, 15:]).all()
    assert list(zip(nb_start[0, :15].tolist(), nb_end[0, :15].tolist())) == \
        [(i, 10) for i in range(5, 10)] + [(10, j) for j in range(10, 21) if j != 14]
    assert not (nb_end[0] == 14).any() and not (nb_start[0] == 14).any()
    assert np.isposinf(lse[0]).all() and np.isfinite(lse[1]).all() and np.isfinite(nb_score[1]).all()
    assert same(out, run(lib, gpu_device, c, 20, 10)), "two runs differ"


# ---- the reader and the command line ----------------------------------------------------------------------------------

def test_reader_forward_n_best(gpu_device):
    from proqa_amd.reader import BertReader, random_state_dict
    from test_reader_gpu import TINY, _pairs
    reader = BertReader.load(random_state_dict(TINY, seed=3, add_select=True), TINY, gpu_device)
    I, S, lens, pos = _pairs(np.random.default_rng(11), 6)
    batch = {"input_ids": torch.from_numpy(I).to(gpu_device), "segment_ids": torch.from_numpy(S).to(gpu_device),
             "seq_lens": lens, "para_offset": pos}
    base = reader.forward(batch, return_logits=True)
    assert reader.forward(batch, return_logits=True, n_best=0).keys() == base.keys()
    out = reader.forward(batch, return_logits=True, n_best=5)
    assert set(out) == set(base) | {"nbest_start", "nbest_end", "nbest_score", "span_lse"}
    B = len(lens)
    assert out["nbest_start"].shape == (B, 5) and out["nbest_start"].dtype == torch.int32
    assert out["nbest_end"].shape == (B, 5) and out["nbest_end"].dtype == torch.int32
    assert out["nbest_score"].shape == (B, 5) and out["nbest_score"].dtype == torch.float32
    assert out["span_lse"].shape == (B, 2) and out["span_lse"].dtype == torch.float32
    for k in ("start", "end", "select", "logits"):
        assert out[k].shape == base[k].shape and out[k].dtype == base[k].dtype and torch.equal(out[k], base[k]), k
    assert torch.equal(out["span_score"].view(torch.int32), base["span_score"].view(torch.int32))
    assert out["cu_seqlens"] == base["cu_seqlens"]
    assert torch.equal(out["start"], out["nbest_start"][:, 0]) and torch.equal(out["end"], out["nbest_end"][:, 0])
    assert torch.equal(out["span_score"], out["nbest_score"][:, 0])
    # the n-best spans score below the best one, and no span's probability under its own passage's norm exceeds 1
    lse = out["span_lse"].sum(1, keepdim=True)
    valid = out["nbest_start"] >= 0
    assert bool(valid.any()) and bool((out["nbest_score"] <= out["nbest_score"][:, :1])[valid].all())
    assert bool((out["nbest_score"] - lse <= 1e-5)[valid].all())


def test_do_predict_n_best_keeps_the_sweep_and_adds_the_marginal_line(gpu_device, tmp_path, monkeypatch):
    from proqa_amd import predict_qa, qa_utils as qu
    from proqa_amd.reader import BertReader
    from test_reader_gpu import _make_world
    tmp = str(tmp_path)
    model_dir, _ = _make_world(tmp)
    argv = ["--do_predict", "--raw-eval-data", f"{tmp}/qa.txt", "--init_checkpoint", f"{tmp}/reader.pt",
            "--index-path", f"{tmp}/embed.npy", "--db-path", f"{tmp}/docs.db", "--index2paraid", f"{tmp}/idx_id.json",
            "--eval-k", "4", "--max_seq_length", "64", "--max_query_length", "10", "--bert_model_name", model_dir,
            "--efficient_eval", "--save-pred", "--prefix", f"{tmp}/pred", "--reader-batch", "5"]

    def cli(extra):
        buf = io.StringIO()
        with redirect_stdout(buf):
            best = predict_qa.main(argv + extra)
        return buf.getvalue().splitlines(), best, dict(predict_qa.LAST_RUN_STATS)

    plain, best0, stats0 = cli([])
    assert "marginal_em" not in stats0 and not os.path.exists(f"{tmp}/pred_marginal.json")
    sweep_files = {a: open(f"{tmp}/pred_{a}.json", "rb").read() for a in qu.ALPHAS}

    # record what the reader returned and what the decoder was given
    forwards, decoded = [], []
    real_forward, real_marginal = BertReader.forward, qu.marginal_answers

    def forward(self, batch, return_logits=False, n_best=0):
        out = real_forward(self, batch, return_logits, n_best)
        forwards.append((n_best, out))
        return out

    def marginal_answers(results, norm):
        decoded.append((results, norm))
        return real_marginal(results, norm)

    monkeypatch.setattr(BertReader, "forward", forward)
    monkeypatch.setattr(qu, "marginal_answers", marginal_answers)
    lines, best, stats = cli(["--n-best", "5", "--marginal", "passage"])
    monkeypatch.undo()

    n_sweep = 2 * len(qu.ALPHAS)
    assert len(plain) == n_sweep + 1 and len(lines) == n_sweep + 2
    assert lines[:n_sweep] == plain[:n_sweep] and lines[-1] == plain[-1] and best == best0
    for a in qu.ALPHAS:
        assert open(f"{tmp}/pred_{a}.json", "rb").read() == sweep_files[a], a

    # the decoder saw the reader's outputs: every valid n-best score and both log-partitions, in sequence order
    assert forwards and all(n == 5 for n, _ in forwards) and all(norm == "passage" for _, norm in decoded)
    valid = torch.cat([o["nbest_start"] for _, o in forwards]).cpu().numpy() >= 0
    scores = torch.cat([o["nbest_score"] for _, o in forwards]).cpu().numpy()
    lses = torch.cat([o["span_lse"] for _, o in forwards]).cpu().numpy()
    qa = [json.loads(l) for l in open(f"{tmp}/qa.txt")]
    qids = [qu.hash_question(q["question"]) for q in qa]
    per_question = {}
    for qid in qids:
        per_question.setdefault(qid, 0)
        per_question[qid] += 4
    assert [len(r) for r, _ in decoded] == list(per_question.values())
    # sequences run question by question; the duplicated last question's passages join the first question's group
    seq_of = {qid: [] for qid in per_question}
    for qi, qid in enumerate(qids):
        seq_of[qid] += list(range(4 * qi, 4 * qi + 4))
    for (results, _), qid in zip(decoded, per_question):
        for x, n in zip(results, seq_of[qid]):
            assert [s for _, s in x["candidates"]] == scores[n][valid[n]].tolist()
            assert np.array_equal(np.asarray(x["lse"], np.float32), lses[n], equal_nan=True)

    # the line and marginal_em are the oracle's decode of those outputs
    ground = {qid: q["answer"] for qid, q in zip(qids, qa)}
    ems = []
    for (results, norm), qid in zip(decoded, per_question):
        ranked = oracle.marginal(results, norm)
        top = ranked[0][2] if ranked else ""
        ems.append(qu.metric_max_over_ground_truths(qu.exact_match_score, top, ground[qid]))
    want = float(np.mean(ems))
    assert stats["marginal_em"] == want
    assert lines[n_sweep] == f"marginal (n-best 5, passage norm): avg. EM: {want}"
    saved = json.load(open(f"{tmp}/pred_marginal.json"))
    assert list(saved) == list(per_question)
    for (results, norm), qid in zip(decoded, per_question):
        ranked = oracle.marginal(results, norm)[:5]
        assert [a["answer"] for a in saved[qid]] == [t for _, _, t in ranked]
        np.testing.assert_allclose([a["prob"] for a in saved[qid]], [p for _, p, _ in ranked], rtol=1e-12)
    assert "postprocess_seconds" in stats and stats["sequences"] == stats0["sequences"]
