"""IndexIVFFlat on the GPU against the NumPy restatement of faiss 1.6.3 IndexIVFFlat (tests/ivf_oracle.py)."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import ivf_oracle

pytestmark = pytest.mark.gpu


def _ivf(nlist, centroids=None, device=None):
    from proqa_amd.index import IndexFlatIP, IndexIVFFlat
    index = IndexIVFFlat(IndexFlatIP(128), 128, nlist)
    if centroids is not None:
        index.set_centroids(torch.from_numpy(np.ascontiguousarray(centroids, np.float32)).to(device))
    return index


def _integer_world(rng, n, nlist, nq):
    """integer-valued rows, queries and centroids (every sum exact in fp32); lists 3 and 9 stay empty (their centroids have
    a negative inner product with every non-negative row), the queries probe them all the same"""
    x = rng.integers(0, 5, (n, 128)).astype(np.float16)
    x[: n // 20] *= 0                      # some all-zero rows: inner-product ties, all go to list 0
    cent = rng.integers(0, 4, (nlist, 128)).astype(np.float32)
    cent[3] = -1
    cent[9] = -2
    xq = rng.integers(-3, 5, (nq, 128)).astype(np.float16)
    return x, cent, xq


@pytest.fixture(scope="module")
def exact_world(gpu_device):
    rng = np.random.default_rng(11)
    nlist = 16
    x, cent, xq = _integer_world(rng, 1500, nlist, 2032)
    index = _ivf(nlist, cent, gpu_device)
    index.add(torch.from_numpy(x).to(gpu_device))
    return index, x, cent, xq


def test_train_follows_the_oracle_trajectory(gpu_device):
    from proqa_amd.index import IndexFlatIP, IndexIVFFlat
    rng = np.random.default_rng(3)
    centers = rng.standard_normal((8, 128)).astype(np.float32) * 3
    x = (centers[rng.integers(0, 8, 3000)] + 0.1 * rng.standard_normal((3000, 128))).astype(np.float16)
    quantizer = IndexFlatIP(128)
    index = IndexIVFFlat(quantizer, 128, 8)          # 3000 > 8 * 256: training sub-samples
    assert not index.is_trained and index.nprobe == 1
    index.train(x)
    cent_o = ivf_oracle.train(x, 8)
    assert index.is_trained and quantizer.ntotal == 8
    np.testing.assert_allclose(index.centroids.cpu().numpy(), cent_o, rtol=1e-4, atol=1e-4)


def test_add_lists_follow_the_oracle_and_several_adds_equal_one(gpu_device, exact_world):
    index, x, cent, _ = exact_world
    a = ivf_oracle.assign(x, cent)
    want = ivf_oracle.lists(a, 16)
    got = index.list_ids()
    assert index.ntotal == len(x)
    for l in range(16):
        np.testing.assert_array_equal(got[l], want[l])
    assert len(want[3]) == 0 and len(want[9]) == 0 and len(want[0]) >= 75
    parts = _ivf(16, cent, gpu_device)
    for r0, r1 in ((0, 1), (1, 700), (700, 701), (701, 1500)):
        parts.add(x[r0:r1])                             # numpy fp16 in pieces
    for l, ids in enumerate(parts.list_ids()):
        np.testing.assert_array_equal(ids, want[l])
    xq = torch.from_numpy(x[:40]).to(gpu_device)
    parts.nprobe = index.nprobe = 16
    for u, v in zip(parts.search_device(xq, 9, inner_products=True), index.search_device(xq, 9, inner_products=True)):
        assert torch.equal(u, v)


@pytest.mark.parametrize("nprobe", [1, 7, 16, 21])
def test_exact_cases_equal_the_oracle_bit_for_bit(gpu_device, exact_world, nprobe):
    index, x, cent, xq = exact_world
    a = ivf_oracle.assign(x, cent)
    Do, Io = ivf_oracle.search(xq, x, a, cent, nprobe, 128)
    index.nprobe = nprobe
    for k in (1, 5, 80, 128):
        for nq in (0, 1, 33, 2032):
            D, I, IP = index.search_device(torch.from_numpy(xq[:nq]).to(gpu_device), k, inner_products=True)
            D, I, IP = D.cpu().numpy(), I.cpu().numpy(), IP.cpu().numpy()
            np.testing.assert_array_equal(I, Io[:nq, :k])
            np.testing.assert_array_equal(D, Do[:nq, :k])
            m = min(nq, 64)
            live = I[:m] >= 0
            ip_o = np.einsum("qd,qkd->qk", xq[:m].astype(np.float64), x[np.maximum(I[:m], 0)].astype(np.float64))
            np.testing.assert_array_equal(IP[:m][live], ip_o[live].astype(np.float32))
            assert (IP[I < 0] == -ivf_oracle.FLT_MAX).all()
    if nprobe == 1:
        assert (Io == -1).any()              # probed lists smaller than k
    st = index.last_stats()
    sizes = index.list_sizes()
    probes = ivf_oracle.coarse(xq, cent, nprobe)
    assert st["nq"] == 2032 and st["lists_probed"] == min(nprobe, 16)
    assert st["rows_scanned"] == int(sizes[probes].sum()) and st["search_ms"] > 0


def test_l2_winner_is_not_the_inner_product_winner(gpu_device):
    from proqa_amd.index import IndexFlatIP
    rng = np.random.default_rng(5)
    x = rng.integers(-2, 3, (300, 128)).astype(np.float16)
    q = rng.integers(-2, 3, (1, 128)).astype(np.float16)
    x[17] = q[0]                 # distance 0, inner product |q|^2
    x[230] = 4 * q[0]            # inner product 4 |q|^2, distance 9 |q|^2
    index = _ivf(4, rng.integers(-1, 2, (4, 128)).astype(np.float32), gpu_device)
    index.add(x)
    index.nprobe = 4
    _, I = index.search(q, 1)
    flat = IndexFlatIP(128)
    flat.add(x)
    _, If = flat.search(q, 1)
    assert I[0, 0] == 17 and If[0, 0] == 230


def _skewed_world(rng, n, nq, nlist=16, clustered=False):
    """fp16 rows; list 0's centroid points along dimension 0, which 30 % of the rows and every query lean on"""
    cent = rng.standard_normal((nlist, 128)).astype(np.float32)
    cent[0] = 0
    cent[0, 0] = 40
    if clustered:
        centers = rng.standard_normal((40, 128)).astype(np.float32) * 2
        x = centers[rng.integers(0, 40, n)] + 0.3 * rng.standard_normal((n, 128)).astype(np.float32)
    else:
        x = rng.standard_normal((n, 128)).astype(np.float32)
    x[: int(0.3 * n), 0] = 4 + rng.random(int(0.3 * n))
    xq = rng.standard_normal((nq, 128)).astype(np.float32)
    xq[:, 0] = 5
    return x.astype(np.float16), cent, xq.astype(np.float16)


@pytest.mark.parametrize("clustered", [False, True])
def test_random_corpora_match_the_oracle(gpu_device, clustered):
    from proqa_amd.index import IndexFlatIP
    rng = np.random.default_rng(7 + clustered)
    x, cent, xq = _skewed_world(rng, 200000, 300, clustered=clustered)
    index = _ivf(16, cent, gpu_device)
    index.add(torch.from_numpy(x).to(gpu_device))
    sizes = index.list_sizes()
    assert sizes[0] >= 0.3 * len(x)                             # one list holds 30 % of the rows (several scan chunks)
    probes = ivf_oracle.coarse(xq, cent, 3)
    assert (probes == 0).any(1).all()                           # ... and every query probes it
    a = np.empty(len(x), np.int64)          # the index's lists (the assignment itself is pinned by the exact cases)
    for l, ids in enumerate(index.list_ids()):
        a[ids] = l
    assert (a != ivf_oracle.assign(x, cent)).sum() <= len(x) // 10000
    index.nprobe = 3
    Do128, Io128 = ivf_oracle.search(xq, x, a, cent, 3, 128)
    for k in (5, 80, 128):
        D, I, IP = (t.cpu().numpy() for t in index.search_device(torch.from_numpy(xq).to(gpu_device), k, inner_products=True))
        Do, Io = Do128[:, :k], Io128[:, :k]
        overlap = np.mean([len(set(I[q]) & set(Io[q])) / k for q in range(len(xq))])
        assert overlap >= 1 - 1e-4, overlap
        np.testing.assert_allclose(D, Do, rtol=1e-5, atol=2e-3)
        # the inner products are IndexFlatIP's scores of those rows, bit for bit
        sample = list(range(0, len(xq), 37))
        union = np.unique(I[sample])
        sub = IndexFlatIP(128)
        sub.add(x[union])
        Ds, Is = sub.search(xq[sample], len(union))
        for n, q in enumerate(sample):
            score = dict(zip(union[Is[n]].tolist(), Ds[n].tolist()))
            np.testing.assert_array_equal(IP[q], np.array([score[i] for i in I[q]], np.float32))
    assert index.last_stats()["chunk_rows"] < sizes[0]


def test_results_repeat_and_do_not_depend_on_the_batch(gpu_device):
    rng = np.random.default_rng(9)
    x, cent, xq = _skewed_world(rng, 240000, 200, clustered=True)
    index = _ivf(16, cent, gpu_device)
    index.add(x)
    index.nprobe = 16
    tq = torch.from_numpy(xq).to(gpu_device)
    first = index.search_device(tq, 80, inner_products=True)
    # >= 59 partial lists per query: its merge runs in batches of 50 lists, later batches often add no key
    assert index.last_stats()["partial_lists"] > 200 * 51
    for _ in range(4):
        again = index.search_device(tq, 80, inner_products=True)
        for u, v in zip(first, again):
            assert torch.equal(u, v)
    for q in range(0, 200, 13):
        alone = index.search_device(tq[q:q + 1], 80, inner_products=True)
        for u, v in zip(first, alone):
            assert torch.equal(u[q:q + 1], v)
    D32, I32 = index.search_device(tq.float(), 80)           # float32 that fp16 holds: the same search
    assert torch.equal(D32, first[0]) and torch.equal(I32, first[1])


def test_refusals(gpu_device):
    from proqa_amd._lib import ProqaError
    rng = np.random.default_rng(2)
    x = rng.standard_normal((600, 128)).astype(np.float32)
    index = _ivf(4)
    with pytest.raises(RuntimeError, match="train"):
        index.search(x[:2].astype(np.float16), 5)
    with pytest.raises(ValueError, match="fp16 cannot hold"):
        index.train(x)                                          # float32 that fp16 cannot hold
    index.train(x.astype(np.float16))
    with pytest.raises(ValueError, match="fp16 cannot hold"):
        index.add(x)
    index.add(x.astype(np.float16))
    with pytest.raises(ProqaError, match="fp16 cannot hold"):
        index.search(x[:3], 5)
    with pytest.raises(ValueError, match="k=129"):
        index.search(x[:3].astype(np.float16), 129)
    index.allow_rounding(True)
    D, I = index.search(x[:3], 5)
    D16, I16 = index.search(x[:3].astype(np.float16), 5)
    np.testing.assert_array_equal(I, I16)


def test_gather_and_online_retriever(gpu_device, exact_world):
    from proqa_amd.online_retriever import OnlineRetriever
    index, x, cent, xq = exact_world
    index.nprobe = 7
    ids = torch.tensor([[5, -1, 1499], [0, 1500, 42]], dtype=torch.int64, device=gpu_device)
    rows = index.reconstruct_batch_device(ids).cpu().numpy()
    want = np.where((ids.cpu().numpy() >= 0)[..., None] & (ids.cpu().numpy() < 1500)[..., None],
                    x[np.clip(ids.cpu().numpy(), 0, 1499)], 0)
    np.testing.assert_array_equal(rows, want)
    np.testing.assert_array_equal(index.reconstruct_batch_device(ids, torch.float32).cpu().numpy(), want.astype(np.float32))
    a = ivf_oracle.assign(x, cent)
    names = [f"p{r}" for r in range(len(x))]
    ret = OnlineRetriever(np.float16, names, index=index)
    for q in (0, 4, 77):
        _, Io = ivf_oracle.search(xq[q:q + 1], x, a, cent, 7, 40)
        idx, pids, embeds = ret.retrieve(torch.from_numpy(xq[q:q + 1]).to(gpu_device), k=40)
        live = Io[0][Io[0] >= 0]
        np.testing.assert_array_equal(idx, live)
        assert pids == [names[i] for i in live]
        np.testing.assert_array_equal(embeds, x[live])


def test_full_size_sampled_queries_equal_a_scan_of_their_probed_lists(gpu_device):
    from proqa_amd.index import IndexFlatIP, IndexIVFFlat
    g = torch.Generator(device=gpu_device).manual_seed(18)
    n, nq, nlist = 18_000_000, 2032, 100
    x = torch.randint(-3, 4, (n, 128), generator=g, device=gpu_device, dtype=torch.int16).half()
    xq = torch.randint(-3, 4, (nq, 128), generator=g, device=gpu_device, dtype=torch.int16).half()
    index = IndexIVFFlat(IndexFlatIP(128), 128, nlist)
    index.train(x)
    index.add(x)
    index.nprobe = 20
    D, I = index.search_device(xq, 80)
    st = index.last_stats()
    lists = index.list_ids()
    assert sum(len(l) for l in lists) == n
    sample = list(range(0, nq, nq // 8))[:8]
    probes = ivf_oracle.coarse(xq[sample].cpu().numpy(), index.centroids.cpu().numpy(), 20)
    rows = 0
    for n_s, q in enumerate(sample):
        cand = torch.from_numpy(np.concatenate([lists[l] for l in probes[n_s]])).to(gpu_device)
        rows += len(cand)
        d = ((x[cand].float() - xq[q].float()) ** 2).sum(1)        # integers below 2^24: exact
        order = torch.argsort(d.double() * n + cand.double())[:80]  # (distance, id), exact in float64
        assert torch.equal(I[q], cand[order])
        assert torch.equal(D[q], d[order])
    assert st["nq"] == nq and st["lists_probed"] == 20 and rows > 0


def test_do_predict_search_ivf_saves_the_oracle_ivf_passage(gpu_device, tmp_path):
    """train_retrieve_qa.py --do_predict --search ivf on test_reader_gpu's synthetic world, with question 0 (and its
    duplicate, question 7) planted so that L2 and inner product disagree: row 11 = q0 (distance 0) and row 21 = 2 q0
    (twice the inner product)."""
    from test_reader_gpu import TINY, _make_world
    from proqa_amd import predict_qa, qa_utils as qu
    from proqa_amd.datasets import TokenizeCollate
    from proqa_amd.reader import BertReader
    from transformers import BertTokenizer
    tmp = str(tmp_path)
    model_dir, sd = _make_world(tmp)
    tok = BertTokenizer.from_pretrained(model_dir)
    reader = BertReader.load(sd, TINY, gpu_device)
    qa = [json.loads(l) for l in open(f"{tmp}/qa.txt")]
    qb = TokenizeCollate(tok, 10)([item["question"] for item in qa])
    q = reader.retriever.get_embed({"input_ids": qb["input_ids"].to(gpu_device), "input_mask": qb["input_mask"].to(gpu_device)},
                                   True, check_mask=False, seq_lens_host=qb["seq_lens"])["embed"].cpu().numpy()
    rng = np.random.default_rng(12)
    emb = (0.01 * rng.standard_normal((30, 128))).astype(np.float16)
    emb[11] = q[0]
    emb[21] = 2 * q[0]
    np.save(f"{tmp}/embed.npy", emb)
    con = __import__("sqlite3").connect(f"{tmp}/docs.db")
    passage = {" ".join(qu.split_words(qu.normalize(qu.normalize(t)))): int(i[3:])
               for i, t in con.execute("SELECT id, text FROM documents")}
    assert len(passage) == 30

    def run(extra, k):
        argv = ["--do_predict", "--raw-eval-data", f"{tmp}/qa.txt", "--init_checkpoint", f"{tmp}/reader.pt",
                "--index-path", f"{tmp}/embed.npy", "--db-path", f"{tmp}/docs.db", "--index2paraid", f"{tmp}/idx_id.json",
                "--eval-k", str(k), "--max_seq_length", "64", "--max_query_length", "10", "--bert_model_name", model_dir,
                "--save-pred", "--prefix", f"{tmp}/pred", "--reader-batch", "5"] + extra
        buf = io.StringIO()
        with redirect_stdout(buf):
            predict_qa.main(argv)
        saved = [json.loads(l) for l in open(f"{tmp}/pred_0.5.json")]
        return buf.getvalue().splitlines(), [passage[s["para"]] for s in saved]

    ivf_args = ["--search", "ivf", "--nlist", "4", "--nprobe", "2"]
    _, rows_ivf = run(ivf_args, 1)
    stats = dict(predict_qa.LAST_RUN_STATS)
    _, rows_exact = run([], 1)
    # the oracle IVF over the same centroids (the command line's training is deterministic: train the same way here)
    index = _ivf(4)
    index.train(emb)
    cent = index.centroids.cpu().numpy()
    a = ivf_oracle.assign(emb, cent)
    qids = list(dict.fromkeys(qu.hash_question(item["question"]) for item in qa))
    first = [[qu.hash_question(item["question"]) for item in qa].index(h) for h in qids]
    _, Io = ivf_oracle.search(q[first], emb, a, cent, 2, 1)
    assert rows_ivf == Io[:, 0].tolist()
    assert rows_ivf[0] == 11 and rows_exact[0] == 21
    assert {"ivf_train_seconds", "ivf_add_seconds", "ivf_search_seconds"} <= set(stats)
    lines, _ = run(ivf_args, 5)
    assert len(lines) == 2 * len(qu.ALPHAS) + 1


def test_stats_cover_every_library_call_and_a_refused_search_reports_zeros(gpu_device, exact_world):
    from proqa_amd._lib import ProqaError
    from proqa_amd.index import IVF_QUERY_BATCH
    index, x, cent, xq = exact_world
    index.nprobe = 7
    many = np.concatenate([xq, xq, xq])[: IVF_QUERY_BATCH + 500]          # two library calls
    index.search_device(torch.from_numpy(many).to(gpu_device), 5)
    st = index.last_stats()
    sizes = index.list_sizes()
    assert st["library_calls"] == 2 and st["nq"] == len(many)
    assert st["rows_scanned"] == int(sizes[ivf_oracle.coarse(many, cent, 7)].sum())
    assert st["search_ms"] > 0 and st["scan_ms"] > 0
    inexact = np.full((2, 128), 0.1, np.float32)                          # fp16 cannot hold 0.1
    with pytest.raises(ProqaError, match="fp16 cannot hold"):
        index.search(inexact, 5)
    st = index.last_stats()
    assert st["nq"] == 0 and st["search_ms"] == 0 and st["library_calls"] == 1
