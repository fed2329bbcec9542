"""Host side of `train_retriever.py --do_predict`: ReDataset / re_collate against the reference's recorded tensors, the
NumPy oracle of the in-batch kernel against the reference's recorded predict, and the refusals of the command line."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import inbatch_oracle
from proqa_amd import datasets

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "retriever_eval_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tokenizer(tmp_path_factory):
    from transformers import BertTokenizer
    d = tmp_path_factory.mktemp("model")
    shutil.copy(os.path.join(GOLDEN, "vocab_small.txt"), d / "vocab.txt")
    return BertTokenizer.from_pretrained(str(d))


@pytest.fixture(scope="module")
def dev_file(gold, tmp_path_factory):
    path = tmp_path_factory.mktemp("dev") / "dev.txt"
    path.write_text("".join(json.dumps(r) + "\n" for r in gold["dataset"]["records"]))
    return str(path)


KEYS = ("input_ids_q", "input_mask_q", "input_ids_c", "input_mask_c")


def test_redataset_and_re_collate_match_the_reference(gold, tokenizer, dev_file):
    g = gold["dataset"]
    for case in g["cases"]:
        ds = datasets.ReDataset(tokenizer, dev_file, case["max_query_length"], case["max_length"])
        assert len(ds) == len(g["records"]) and ds.group_indexs == case["group_indexs"]
        samples = [ds[i] for i in range(len(ds))]
        assert [int(s["input_ids_q"].numel()) for s in samples] == case["item_lengths_q"]
        assert [int(s["input_ids_c"].numel()) for s in samples] == case["item_lengths_c"]
        assert all(s["input_mask_q"].dtype == torch.bool and bool(s["input_mask_q"].all()) and
                   s["input_mask_c"].dtype == torch.bool and bool(s["input_mask_c"].all()) for s in samples)
        batch = datasets.re_collate(samples)
        assert batch["input_ids_q"].dtype == torch.int64 and batch["input_mask_c"].dtype == torch.bool
        for k in KEYS:
            assert batch[k].int().tolist() == case[k], k
    assert datasets.re_collate([]) == {}


def test_filter_sample_and_the_filtered_dataset_match_the_reference(gold, tokenizer, dev_file):
    g = gold["dataset"]
    ds = datasets.ReDataset(tokenizer, dev_file, 6, 22)
    assert [ds.filter_sample(r) for r in g["records"]] == g["filter_sample"]
    kept = datasets.ReDataset(tokenizer, dev_file, 6, 22, filter=True)
    assert len(kept) == g["filtered_len"] == sum(g["filter_sample"])
    assert [r["Question"] for r in kept.data] == [r["Question"] for r, keep in zip(g["records"], g["filter_sample"]) if keep]
    assert sorted(sum(kept.group_indexs, [])) == list(range(len(kept)))


@pytest.mark.parametrize("native_threads", [0, 2])
def test_the_batch_collate_of_the_command_line_gives_the_same_tensors(gold, tokenizer, dev_file, native_threads):
    """ReTokenizeCollate over the strings (the tokenizer library's batch call, or the native WordPiece) == re_collate over
    the items, in batches of 7 with a short last one."""
    g = gold["dataset"]
    for case in g["cases"]:
        ds = datasets.ReDataset(tokenizer, dev_file, case["max_query_length"], case["max_length"])
        view = datasets.ReTextView(ds)
        collate = datasets.ReTokenizeCollate(tokenizer, case["max_query_length"], case["max_length"],
                                             native_threads=native_threads)
        assert (collate.q.has_native and collate.c.has_native) == (native_threads > 0)
        for b0 in range(0, len(ds), 7):
            idx = range(b0, min(b0 + 7, len(ds)))
            want = datasets.re_collate([ds[i] for i in idx])
            got = collate([view[i] for i in idx])
            for k in KEYS:
                assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (k, b0)
            assert got["seq_lens_q"] == want["input_mask_q"].sum(1).tolist()
            assert got["seq_lens_c"] == want["input_mask_c"].sum(1).tolist()
    assert collate([]) == {}


def test_the_oracle_reproduces_the_reference_predict(gold):
    p = gold["predict"]
    batches = [(np.asarray(q, np.float16), np.asarray(c, np.float16)) for q, c in zip(p["q"], p["c"])]
    assert [len(q) for q, _ in batches] == [7, 7, 3]
    num_total, acc, argmaxes = inbatch_oracle.predict_accounting(batches)
    assert [a.tolist() for a in argmaxes] == p["argmax"]
    assert num_total == p["num_total"] and acc == p["acc"] and 0.0 < acc < 1.0
    assert f"evaluated {num_total} examples..." == p["first_line"]
    assert f"avg. Acc: {acc}" == p["second_line_reference"]
    # the planted ties: batch 0 holds one paragraph at columns 2 and 5
    o = inbatch_oracle.inbatch_eval(*batches[0])
    assert o["scores"][5, 2] == o["scores"][5, 5] and o["argmax"][5] == 2 and o["rank"][5] == 1    # gold ties with a lower column
    assert o["scores"][2, 2] == o["scores"][2, 5] and o["argmax"][2] == 2 and o["rank"][2] == 0    # ... with a higher one
    o = inbatch_oracle.inbatch_eval(*batches[1])
    assert o["argmax"][1] == 4 and o["rank"][1] >= 1


def test_the_oracle_follows_torch_on_ties_and_non_finite_scores():
    """argmax and logsumexp of the oracle against torch on the CPU (the reference's arithmetic), on rows with ties, NaN
    and infinities."""
    inf, nan = float("inf"), float("nan")
    s = np.array([[1.0, 3.0, 3.0, 2.0], [nan, 5.0, nan, 1.0], [2.0, nan, 9.0, inf], [-inf, -inf, -inf, -inf],
                  [1.0, inf, inf, 0.0], [0.0, -0.0, -1.0, -inf], [3e4, -3e4, 2.9e4, 0.0]])
    t = torch.from_numpy(s)
    assert inbatch_oracle.argmax_lowest(s).tolist() == t.argmax(-1).tolist() == [1, 0, 1, 0, 1, 0, 0]
    want = torch.logsumexp(t, -1).numpy()
    got = inbatch_oracle.logsumexp(s)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).tolist() == [False, True, True] + [False] * 4
    ok = ~np.isnan(got)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-15, atol=0)
    assert got[3] == -inf and got[4] == inf
    # rank: NaN beats every number, ties count from the left only
    target = np.array([2, 3, 2, 1, 2, 1, 2])
    assert inbatch_oracle.rank_of_gold(s, target).tolist() == [1, 3, 2, 1, 1, 1, 1]
    assert inbatch_oracle.rank_of_gold(s[1:2], np.array([2])).tolist() == [1]      # a NaN gold: only the NaN to its left


def test_gaussian_cases_of_the_gpu_test_exclude_no_row():
    """The seeds of tests/test_inbatch_gpu.py: in float64 every row's top-1 / top-2 margin and the distance from the gold
    to the nearest other score exceed twice the fp32 accumulation bound, so the oracle alone excludes nothing."""
    import test_inbatch_gpu as t
    for nq, nc in t.GAUSSIAN_SHAPES:
        q, c, target = t.gaussian_case(nq, nc)
        keep_argmax, keep_rank, bound = t.decided_rows(q, c, target)
        assert keep_argmax.all() and keep_rank.all(), (nq, nc)
        assert bound.max() < 1e-3


def test_command_line_refusals(tmp_path):
    from proqa_amd import train_retriever
    dev = tmp_path / "dev.txt"
    dev.write_text(json.dumps({"Question": "q", "Paragraph": "p"}) + "\n")
    with pytest.raises(SystemExit, match=r"--do_train is not supported: this project runs the retriever's evaluation "
                                         r"\(--do_predict\) only; train with the reference"):
        train_retriever.main(["--do_train", "--train_file", "x", "--predict_file", str(dev)])
    with pytest.raises(ValueError, match="If `do_predict` is True, then `predict_file` must be specified."):
        train_retriever.main(["--do_predict", "--init_checkpoint", "ckpt.pt"])
    with pytest.raises(SystemExit, match="';' list in --init_checkpoint"):
        train_retriever.main(["--do_predict", "--predict_file", str(dev), "--init_checkpoint", "a.pt;b.pt"])
    with pytest.raises(ValueError, match="At least one of `do_train` or `do_predict` must be True."):
        train_retriever.main(["--predict_file", str(dev)])
    with pytest.raises(SystemExit, match="needs --init_checkpoint"):
        train_retriever.main(["--do_predict", "--predict_file", str(dev)])


def test_root_script_is_the_module_entry_point():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_retriever_root", os.path.join(root, "train_retriever.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from proqa_amd import train_retriever
    assert mod.main is train_retriever.main
