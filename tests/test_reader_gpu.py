"""Reader path on the GPU: typed embeddings, the fused span kernel, the reader forward and the --do_predict command line.

Tolerances: the reader tower is the retriever's encoder (fp16 storage, fp32 accumulation) with token types, compared
with the fp32 NumPy oracle at the per-kernel / small-model tolerances of test_encoder_gpu.py.  The span choice is exact:
the kernel's (start, end, score bits) must equal a NumPy enumeration of every (i, j) pair over the kernel's OWN logits.
"""
import ctypes
import io
import json
import os
import sqlite3
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from reader_oracle import brute_span, typed_tower

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev16(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=torch.float16)


@pytest.fixture(scope="module")
def lib(gpu_device):
    from proqa_amd import _lib
    return _lib.load()


def _ln(x, g, b, eps=1e-12):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


@pytest.mark.parametrize("hidden,S,B,n_types", [(128, 40, 5, 2), (768, 77, 3, 2), (1024, 9, 2, 3)])
def test_typed_embed_layernorm_padded_and_packed(lib, gpu_device, hidden, S, B, n_types):
    from proqa_amd import _lib
    rng = np.random.default_rng(hidden + S)
    vocab = 700
    word = rng.standard_normal((vocab, hidden)).astype(np.float16)
    pos = rng.standard_normal((S, hidden)).astype(np.float16)
    types = rng.standard_normal((n_types, hidden)).astype(np.float16)
    g = (1 + 0.1 * rng.standard_normal(hidden)).astype(np.float16)
    b = (0.1 * rng.standard_normal(hidden)).astype(np.float16)
    ids = rng.integers(0, vocab, (B, S)).astype(np.int64)
    tt = rng.integers(0, n_types, (B, S)).astype(np.int64)
    ref = _ln(word.astype(np.float32)[ids] + pos.astype(np.float32)[None] + types.astype(np.float32)[tt],
              g.astype(np.float32), b.astype(np.float32))
    d = gpu_device
    W, P, T, G, Bt = (dev16(a, d) for a in (word, pos, types, g, b))
    ids_d, tt_d = torch.from_numpy(ids).to(d), torch.from_numpy(tt).to(d)
    out = torch.empty((B * S, hidden), dtype=torch.float16, device=d)
    _lib.check(lib.proqa_embed_layernorm_typed_f16(ids_d.data_ptr(), tt_d.data_ptr(), B * S, S, hidden, W.data_ptr(), vocab,
                                                   P.data_ptr(), T.data_ptr(), n_types, G.data_ptr(), Bt.data_ptr(), 1e-12,
                                                   out.data_ptr(), stream()))
    np.testing.assert_allclose(out.float().cpu().numpy().reshape(B, S, hidden), ref, rtol=2e-3, atol=2e-3)
    # NULL type ids = all type 0
    _lib.check(lib.proqa_embed_layernorm_typed_f16(ids_d.data_ptr(), None, B * S, S, hidden, W.data_ptr(), vocab,
                                                   P.data_ptr(), T.data_ptr(), n_types, G.data_ptr(), Bt.data_ptr(), 1e-12,
                                                   out.data_ptr(), stream()))
    ref0 = _ln(word.astype(np.float32)[ids] + pos.astype(np.float32)[None] + types.astype(np.float32)[0],
               g.astype(np.float32), b.astype(np.float32))
    np.testing.assert_allclose(out.float().cpu().numpy().reshape(B, S, hidden), ref0, rtol=2e-3, atol=2e-3)
    # packed
    lens = rng.integers(1, S + 1, B).astype(np.int32)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cu_d = torch.from_numpy(cu).to(d)
    packed = torch.full((int(cu[-1]) + 1, hidden), 7.0, dtype=torch.float16, device=d)
    _lib.check(lib.proqa_embed_layernorm_typed_varlen_f16(ids_d.data_ptr(), tt_d.data_ptr(), cu_d.data_ptr(), B, S, hidden,
                                                          W.data_ptr(), vocab, P.data_ptr(), T.data_ptr(), n_types,
                                                          G.data_ptr(), Bt.data_ptr(), 1e-12, packed.data_ptr(), stream()))
    got = packed.float().cpu().numpy()
    for k in range(B):
        np.testing.assert_allclose(got[cu[k]:cu[k + 1]], ref[k, :lens[k]], rtol=2e-3, atol=2e-3)
    assert (got[-1] == 7.0).all(), "the packed embedding wrote past its last token"


def _run_span(lib, d, hidden, lens, para_offset, qa_w, qa_b, max_len, padded=False, mal=10):
    from proqa_amd import _lib
    B = len(lens)
    H = hidden.shape[1]
    lens_t = torch.tensor(lens, dtype=torch.int32, device=d)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=d)
    po = torch.tensor(para_offset, dtype=torch.int32, device=d)
    rows = hidden.shape[0]
    start = torch.full((B,), -7, dtype=torch.int32, device=d)
    end = torch.full((B,), -7, dtype=torch.int32, device=d)
    score = torch.zeros(B, dtype=torch.float32, device=d)
    logits = torch.full((rows + 1, 2), 3.0, dtype=torch.float16, device=d)    # one guard row
    _lib.check(lib.proqa_reader_span_f16(hidden.data_ptr(), lens_t.data_ptr() if padded else None,
                                         None if padded else cu.data_ptr(), B, max_len, H, po.data_ptr(), qa_w.data_ptr(),
                                         qa_b.data_ptr(), mal, start.data_ptr(), end.data_ptr(), score.data_ptr(),
                                         logits.data_ptr(), stream()))
    lg = logits.float().cpu().numpy()
    assert (lg[-1] == 3.0).all(), "span kernel wrote past the last row's logits"
    return start.cpu().numpy(), end.cpu().numpy(), score.cpu().numpy(), lg[:-1]


def _check_spans(start, end, score, lg, row0s, lens, para_offset, mal=10):
    for b in range(len(lens)):
        r0 = row0s[b]
        bi, bj, bs = brute_span(lg[r0:r0 + lens[b], 0], lg[r0:r0 + lens[b], 1], para_offset[b], lens[b], mal)
        assert (start[b], end[b]) == (bi, bj), (b, lens[b], para_offset[b], (start[b], end[b]), (bi, bj))
        assert np.float32(score[b]).view(np.int32) == np.float32(bs).view(np.int32), (b, score[b], bs)


@pytest.mark.parametrize("H", [768, 128])
def test_span_kernel_random_mixed_batch(lib, gpu_device, H):
    d = gpu_device
    rng = np.random.default_rng(H)
    # lengths that are multiples of nothing, 512, a sequence of only [CLS] q [SEP] [SEP] (no paragraph token), tiny ones
    lens = [512, 3, 37, 129, 4, 511, 200, 5, 300, 1, 2]
    para_offset = [9, 2, 12, 4, 3, 30, 199, 3, 298, 0, 1]
    T = sum(lens)
    hid = dev16(rng.standard_normal((T, H)), d)
    qa_w = dev16(rng.standard_normal((2, H)) * 0.2, d)
    qa_b = dev16(rng.standard_normal(2) * 0.1, d)
    start, end, score, lg = _run_span(lib, d, hid, lens, para_offset, qa_w, qa_b, 512)
    row0s = np.concatenate([[0], np.cumsum(lens)])
    _check_spans(start, end, score, lg, row0s, lens, para_offset)
    # empty paragraphs
    for b in range(len(lens)):
        if para_offset[b] >= lens[b] - 1:
            assert start[b] == -1 and end[b] == -1 and np.isneginf(score[b])
    # the logits are a half-precision Linear of the hidden rows
    h32 = hid.float().cpu().numpy()
    ref = h32 @ qa_w.float().cpu().numpy().T + qa_b.float().cpu().numpy()
    np.testing.assert_allclose(lg, ref, rtol=2e-3, atol=2e-3 * max(1.0, float(np.abs(ref).max()) / 8))
    # padded layout, same sequences: the same answers and logits
    S = 512
    pad = torch.zeros((len(lens) * S, H), dtype=torch.float16, device=d)
    for b in range(len(lens)):
        pad[b * S:b * S + lens[b]] = hid[row0s[b]:row0s[b + 1]]
    s2, e2, sc2, lg2 = _run_span(lib, d, pad, lens, para_offset, qa_w, qa_b, S, padded=True)
    assert (s2 == start).all() and (e2 == end).all() and (sc2.view(np.int32) == score.view(np.int32)).all()
    for b in range(len(lens)):
        assert (lg2[b * S:b * S + lens[b]] == lg[row0s[b]:row0s[b + 1]]).all()


def test_span_kernel_planted_ties_and_edges(lib, gpu_device):
    """Hidden rows built so that the logits are exact small integers: planted equal scores must resolve to the lowest
    start, then the lowest end; spans at the first and last paragraph positions; max_answer_len 0 and 30."""
    d = gpu_device
    H = 128
    rng = np.random.default_rng(7)
    # qa_w = unit vectors on columns 0 / 1: start logit = hidden[:, 0], end logit = hidden[:, 1] (exact)
    w = np.zeros((2, H), np.float32)
    w[0, 0] = 1.0
    w[1, 1] = 1.0
    qa_w, qa_b = dev16(w, d), dev16(np.zeros(2), d)
    cases = []
    # (lens, para_offset, start logits, end logits)
    L = 64
    s = rng.integers(-3, 3, L).astype(np.float32)
    e = rng.integers(-3, 3, L).astype(np.float32)
    cases.append((L, 5, s, e))                      # many ties among small integers
    s = np.zeros(L, np.float32)
    e = np.zeros(L, np.float32)
    cases.append((L, 5, s, e))                      # all equal: (po, po)
    s = np.full(L, -5.0, np.float32)
    e = np.full(L, -5.0, np.float32)
    s[62] = 4.0
    e[62] = 4.0                                      # the last paragraph position (len - 2)
    e[63] = 100.0                                    # the final [SEP] must not count
    cases.append((L, 5, s, e))
    s = np.full(L, -5.0, np.float32)
    e = np.full(L, -5.0, np.float32)
    s[5], e[15], e[16] = 2.0, 3.0, 3.0               # answer exactly max_answer_len long; 16 is one too far
    s[4] = 50.0                                      # before the paragraph: masked
    cases.append((L, 5, s, e))
    s = rng.integers(-2, 2, 512).astype(np.float32)
    e = rng.integers(-2, 2, 512).astype(np.float32)
    cases.append((512, 20, s, e))
    lens = [c[0] for c in cases]
    po = [c[1] for c in cases]
    T = sum(lens)
    hid = np.zeros((T, H), np.float32)
    hid[:, 2:] = rng.standard_normal((T, H - 2))      # noise the weights ignore
    r = 0
    for L_, _, s_, e_ in cases:
        hid[r:r + L_, 0] = s_
        hid[r:r + L_, 1] = e_
        r += L_
    hid_d = dev16(hid, d)
    row0s = np.concatenate([[0], np.cumsum(lens)])
    for mal in (10, 0, 30):
        start, end, score, lg = _run_span(lib, d, hid_d, lens, po, qa_w, qa_b, 512, mal=mal)
        np.testing.assert_array_equal(lg[:, 0], hid[:, 0])
        np.testing.assert_array_equal(lg[:, 1], hid[:, 1])
        _check_spans(start, end, score, lg, row0s, lens, po, mal)
    start, end, score, _ = _run_span(lib, d, hid_d, lens, po, qa_w, qa_b, 512, mal=10)
    assert (start[1], end[1]) == (5, 5)
    assert (start[2], end[2]) == (62, 62) and score[2] == 8.0
    assert (start[3], end[3]) == (5, 15) and score[3] == 5.0


TINY = dict(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512,
            max_position_embeddings=128, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")


def _pairs(rng, n, L_max=100, vocab=512):
    ids, segs, lens, pos = [], [], [], []
    for _ in range(n):
        q = int(rng.integers(3, 12))
        L = int(rng.integers(q + 1, L_max + 1))
        x = rng.integers(110, vocab, L)
        x[0], x[q - 1], x[L - 1] = 101, 102, 102
        ids.append(x)
        segs.append(np.r_[np.zeros(q, np.int64), np.ones(L - q, np.int64)])
        lens.append(L)
        pos.append(q)
    W = max(lens)
    I = np.zeros((n, W), np.int64)
    S = np.zeros((n, W), np.int64)
    for k in range(n):
        I[k, :lens[k]] = ids[k]
        S[k, :lens[k]] = segs[k]
    return I, S, lens, pos


@pytest.mark.parametrize("add_select", [False, True])
def test_reader_forward_vs_numpy_oracle(gpu_device, add_select):
    from proqa_amd.reader import BertReader, random_state_dict
    sd = random_state_dict(TINY, seed=3, add_select=add_select)
    reader = BertReader.load(sd, TINY, gpu_device)
    rng = np.random.default_rng(11)
    I, S, lens, pos = _pairs(rng, 6)
    out = reader.forward({"input_ids": torch.from_numpy(I).to(gpu_device), "segment_ids": torch.from_numpy(S).to(gpu_device),
                          "seq_lens": lens, "para_offset": pos}, return_logits=True)
    sdn = {k: v.numpy() for k, v in sd.items()}
    mask = np.arange(I.shape[1])[None] < np.asarray(lens)[:, None]
    hidden, pooled = typed_tower(sdn, "bert", I, S, mask, TINY["num_hidden_layers"], TINY["num_attention_heads"])
    lg = out["logits"].float().cpu().numpy()
    cu = out["cu_seqlens"]
    for b in range(len(lens)):
        ref = hidden[b, :lens[b]] @ sdn["qa_outputs.weight"].T + sdn["qa_outputs.bias"]
        np.testing.assert_allclose(lg[cu[b]:cu[b + 1]], ref, rtol=2e-3, atol=2e-3)
    start, end, score = (out[k].cpu().numpy() for k in ("start", "end", "span_score"))
    _check_spans(start, end, score, lg, cu, lens, pos)
    if add_select:
        ref = pooled @ sdn["select_outputs.weight"].T[:, 0] + sdn["select_outputs.bias"][0]
        np.testing.assert_allclose(out["select"].cpu().numpy(), ref, rtol=2e-3, atol=2e-3)
    else:
        assert out["select"] is None


def test_reader_forward_vs_reference_golden(gpu_device):
    """BertRetrieveQA.forward of the reference itself (fp32, reader_forward_golden.npz from make_reader_golden.py):
    start / end logits on the paragraph, the select head, and the rank logit q . para_embed of the question tower, at
    the small-model tolerances of test_encoder_gpu.py (fp16 storage, fp32 accumulation; logits ~0.1-3)."""
    from proqa_amd.reader import BertReader
    z = np.load(os.path.join(GOLDEN, "reader_forward_golden.npz"))
    cfg = json.loads(str(z["config"]))
    sd = {k[3:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w::")}
    reader = BertReader.load(sd, cfg, gpu_device)
    assert reader.add_select
    lens, po = z["seq_lens"].tolist(), z["para_offset"].tolist()
    out = reader.forward({"input_ids": torch.from_numpy(z["input_ids"]).to(gpu_device),
                          "segment_ids": torch.from_numpy(z["segment_ids"]).to(gpu_device), "seq_lens": lens,
                          "para_offset": po}, return_logits=True)
    lg = out["logits"].float().cpu().numpy()
    cu = out["cu_seqlens"]
    for b in range(len(lens)):
        par = slice(po[b], lens[b] - 1)          # the reference masks everything else with -1e10
        np.testing.assert_allclose(lg[cu[b]:cu[b + 1]][par, 0], z["start_logits"][b, par], rtol=3e-3, atol=3e-3)
        np.testing.assert_allclose(lg[cu[b]:cu[b + 1]][par, 1], z["end_logits"][b, par], rtol=3e-3, atol=3e-3)
    np.testing.assert_allclose(out["select"].cpu().numpy(), z["select_logits"].reshape(-1), rtol=3e-3, atol=3e-3)
    q_ids = torch.from_numpy(z["input_ids_q"]).to(gpu_device)
    q = reader.retriever.get_embed({"input_ids": q_ids, "input_mask": torch.ones_like(q_ids, dtype=torch.bool)},
                                   True)["embed"].float().cpu().numpy()
    np.testing.assert_allclose(q @ z["para_embed"].T, z["rank_logits"], rtol=5e-3, atol=5e-3)


def test_reader_spans_do_not_depend_on_batch_composition(gpu_device):
    from proqa_amd.reader import BertReader, random_state_dict
    sd = random_state_dict(TINY, seed=5)
    sd["qa_outputs.weight"] = sd["qa_outputs.weight"] * 50     # wide logit margins: fp16 noise cannot flip a choice
    reader = BertReader.load(sd, TINY, gpu_device)
    rng = np.random.default_rng(2)
    I, S, lens, pos = _pairs(rng, 9)

    def run(rows):
        W = max(lens[r] for r in rows)
        return reader.forward({"input_ids": torch.from_numpy(I[rows, :W]).to(gpu_device),
                               "segment_ids": torch.from_numpy(S[rows, :W]).to(gpu_device),
                               "seq_lens": [lens[r] for r in rows], "para_offset": [pos[r] for r in rows]},
                              return_logits=True)
    full = run(list(range(9)))
    lg = full["logits"].float().cpu().numpy()
    margin_ok = []
    for b in range(9):
        c0 = full["cu_seqlens"][b]
        s, e = lg[c0:c0 + lens[b], 0], lg[c0:c0 + lens[b], 1]
        scores = sorted({float(s[i] + e[j]) for i in range(pos[b], lens[b] - 1) for j in range(i, min(i + 10, lens[b] - 2) + 1)},
                        reverse=True)
        margin_ok.append(len(scores) < 2 or scores[0] - scores[1] > 0.05 * max(1.0, abs(scores[0])))
    assert sum(margin_ok) >= 5
    for rows in ([4], [8, 0, 3], list(range(8, -1, -1))):
        part = run(rows)
        for k, r in enumerate(rows):
            if margin_ok[r]:
                assert int(part["start"][k]) == int(full["start"][r]) and int(part["end"][k]) == int(full["end"][r])


def test_encoder_without_projection_refuses_forward(gpu_device):
    from proqa_amd import _lib
    from proqa_amd.retriever import _Tower, config_from_dict
    from proqa_amd.reader import random_state_dict
    cfg = config_from_dict(TINY)
    tw = _Tower(random_state_dict(TINY), "bert", None, cfg, gpu_device)
    lib = _lib.load()
    ids = torch.ones((1, 4), dtype=torch.int64, device=gpu_device)
    lens = torch.tensor([4], dtype=torch.int32, device=gpu_device)
    out = torch.empty((1, 128), dtype=torch.float16, device=gpu_device)
    rc = lib.proqa_encoder_forward(tw._handle, ids.data_ptr(), lens.data_ptr(), 1, 4, 4, 0, out.data_ptr(), 0, stream())
    assert rc == -1 and b"no projection" in lib.proqa_last_error()
    tw.close()


# ---- end to end: the command line ------------------------------------------------------------------------------------

def _make_world(tmp, n_paras=30, n_q=7):
    """tiny model dir (config + vocab), random reader checkpoint, DocDB, index, id map, questions"""
    from proqa_amd.reader import random_state_dict
    model_dir = os.path.join(tmp, "model")
    os.makedirs(model_dir)
    with open(os.path.join(model_dir, "config.json"), "w") as f:
        json.dump(dict(TINY, model_type="bert"), f)
    vocab = [l.rstrip("\n") for l in open(os.path.join(GOLDEN, "vocab_small.txt"))]
    with open(os.path.join(model_dir, "vocab.txt"), "w") as f:
        f.write("\n".join(vocab) + "\n")
    sd = random_state_dict(TINY, seed=9)
    # equal start and end heads: the best span is then the single best piece (max s_i + s_j over j >= i is at i = j), so a
    # one-word gold answer can match and the printed EMs carry signal
    sd["qa_outputs.weight"][1] = sd["qa_outputs.weight"][0]
    sd["qa_outputs.bias"][1] = sd["qa_outputs.bias"][0]
    torch.save({"module." + k: v for k, v in sd.items()}, os.path.join(tmp, "reader.pt"))
    rng = np.random.default_rng(4)
    words = [w for w in vocab if w.isalpha() and len(w) > 1 and not w.startswith("tok")]
    paras = []
    for p in range(n_paras):
        n = 0 if p == 1 else int(rng.integers(3, 60))
        paras.append(" ".join(rng.choice(words, n)) + ("" if p % 5 else " Paris France, tête-à-tête"))
    db = os.path.join(tmp, "docs.db")
    con = sqlite3.connect(db)
    con.execute("CREATE TABLE documents (id PRIMARY KEY, text)")
    con.executemany("INSERT INTO documents VALUES (?, ?)", [(f"doc{p}", t) for p, t in enumerate(paras)])
    con.commit()
    con.close()
    emb = rng.standard_normal((n_paras, 128)).astype(np.float16)
    np.save(os.path.join(tmp, "embed.npy"), emb)
    with open(os.path.join(tmp, "idx_id.json"), "w") as f:
        json.dump({str(p): f"doc{p}" for p in range(n_paras)}, f)
    qs = []
    for q in range(n_q):
        qs.append({"question": " ".join(rng.choice(words, int(rng.integers(2, 8)))), "answer": list(words) + ["paris"]})
    # (every single vocabulary word is a gold answer: a one-word span of the random reader scores, so EM is not all 0)
    qs.append(dict(qs[0]))                   # a duplicated question: grouped by its hash
    with open(os.path.join(tmp, "qa.txt"), "w") as f:
        for q in qs:
            f.write(json.dumps(q) + "\n")
    return model_dir, sd


def test_do_predict_command_line_matches_host_sweep_over_gpu_logits(gpu_device, tmp_path):
    from proqa_amd import predict_qa, qa_utils as qu
    from proqa_amd.reader import BertReader
    from transformers import BertTokenizer
    tmp = str(tmp_path)
    model_dir, sd = _make_world(tmp)
    argv = ["--do_predict", "--raw-eval-data", f"{tmp}/qa.txt", "--init_checkpoint", f"{tmp}/reader.pt",
            "--index-path", f"{tmp}/embed.npy", "--db-path", f"{tmp}/docs.db", "--index2paraid", f"{tmp}/idx_id.json",
            "--eval-k", "4", "--max_seq_length", "64", "--max_query_length", "10", "--bert_model_name", model_dir,
            "--efficient_eval", "--save-pred", "--prefix", f"{tmp}/pred", "--reader-batch", "5"]
    buf = io.StringIO()
    with redirect_stdout(buf):
        predict_qa.main(argv)
    lines = buf.getvalue().splitlines()
    assert len(lines) == 2 * len(qu.ALPHAS) + 1

    # the same evaluation, host-only from the GPU's logits: search, pairs, NumPy spans, sweep
    tok = BertTokenizer.from_pretrained(model_dir)
    reader = BertReader.load(sd, TINY, gpu_device)
    qa = [json.loads(l) for l in open(f"{tmp}/qa.txt")]
    emb = np.load(f"{tmp}/embed.npy").astype(np.float32)
    idmap = json.load(open(f"{tmp}/idx_id.json"))
    con = sqlite3.connect(f"{tmp}/docs.db")
    cls_id, sep_id = tok.convert_tokens_to_ids("[CLS]"), tok.convert_tokens_to_ids("[SEP]")
    # the questions as the command line encodes them: one padded batch (fewer than 256), packed by the encoder
    from proqa_amd.datasets import TokenizeCollate
    qb = TokenizeCollate(tok, 10)([item["question"] for item in qa])
    q_all = reader.retriever.get_embed({"input_ids": qb["input_ids"].to(gpu_device), "input_mask": qb["input_mask"].to(gpu_device)},
                                       True, check_mask=False, seq_lens_host=qb["seq_lens"])["embed"].float().cpu().numpy()
    pairs = []
    for qi, item in enumerate(qa):
        q_ids = tok.encode(item["question"], max_length=10, truncation=True)
        q = q_all[qi]
        sc = emb.astype(np.float64) @ q.astype(np.float64)
        rows = sorted(range(len(sc)), key=lambda r: (-sc[r], r))[:4]
        for r in rows:
            text = qu.normalize(con.execute("SELECT text FROM documents WHERE id = ?", (idmap[str(r)],)).fetchone()[0])
            words = qu.split_words(text)
            pieces, t2o = [], []
            for wi, w in enumerate(words):
                p = tok.tokenize(w)
                pieces += p
                t2o += [wi] * len(p)
            ids, seg, po, _ = qu.build_pair(q_ids, tok.convert_tokens_to_ids(pieces), 64, cls_id, sep_id)
            pairs.append((item, float(np.float32(sc[r])), words, pieces, t2o, ids, seg, po))
    qid2results, qid2ground = {}, {}
    for b0 in range(0, len(pairs), 5):      # the command line's --reader-batch 5: the same GEMM shapes, the same logits
        chunk = pairs[b0:b0 + 5]
        W = max(len(c[5]) for c in chunk)
        I = np.zeros((len(chunk), W), np.int64)
        S = np.zeros((len(chunk), W), np.int64)
        for k, c in enumerate(chunk):
            I[k, :len(c[5])], S[k, :len(c[6])] = c[5], c[6]
        out = reader.forward({"input_ids": torch.from_numpy(I).to(gpu_device), "segment_ids": torch.from_numpy(S).to(gpu_device),
                              "seq_lens": [len(c[5]) for c in chunk], "para_offset": [c[7] for c in chunk]}, return_logits=True)
        lg = out["logits"].float().cpu().numpy()
        for k, (item, rank, words, pieces, t2o, ids, seg, po) in enumerate(chunk):
            c0 = out["cu_seqlens"][k]
            bi, bj, bs = brute_span(lg[c0:c0 + len(ids), 0], lg[c0:c0 + len(ids), 1], po, len(ids))
            qid = qu.hash_question(item["question"])
            qid2results.setdefault(qid, []).append({
                "text": qu.answer_text(bi, bj, po, words, pieces, t2o), "rank_score": rank,
                "span_score": float(bs) if bi >= 0 else None, "passage": " ".join(words), "question": item["question"]})
            qid2ground[qid] = item["answer"]
    want = []
    _, best = qu.alpha_sweep(qid2results, qid2ground, out=want.append)
    assert lines[:-1] == want
    assert lines[-1] == str(best)
    assert lines[0] == f"evaluated {len(qid2results)} examples..."
    assert any(float(l.split("EM: ")[1]) > 0 for l in lines if "EM: " in l), lines
    assert os.path.exists(f"{tmp}/pred_0.5.json")
