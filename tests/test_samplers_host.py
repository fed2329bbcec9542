"""The training loop's samplers (proqa_amd.datasets.ReSampler, ClusterDataset, ClusterSampler) against the reference's own
classes: tests/golden/sampler_golden.json holds the index orders the reference's samplers gave over
tests/golden/sampler_inputs/ for two seeds of `random` and `np.random` (tests/golden/make_sampler_golden.py)."""
import collections
import json
import os
import random
import shutil

import numpy as np
import pytest
import torch

from proqa_amd import datasets

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
INPUTS = os.path.join(GOLDEN, "sampler_inputs")
TRAIN = os.path.join(INPUTS, "train.txt")
CLUSTERS = os.path.join(INPUTS, "clusters")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "sampler_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tokenizer(tmp_path_factory):
    from transformers import BertTokenizer
    d = tmp_path_factory.mktemp("model")
    shutil.copy(os.path.join(GOLDEN, "vocab_small.txt"), d / "vocab.txt")
    return BertTokenizer.from_pretrained(str(d))


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


def test_inputs_are_the_documented_ones():
    assert sum(1 for _ in open(TRAIN)) == 10
    assert [sum(1 for _ in open(os.path.join(CLUSTERS, f))) for f in sorted(os.listdir(CLUSTERS))] == [4, 7, 9]


def test_re_sampler_gives_the_reference_order(gold):
    for seed in gold["seeds"]:
        seed_all(seed)
        ds = datasets.ReDataset(None, TRAIN, 8, 32)
        sampler = datasets.ReSampler(ds)
        order = list(sampler)
        assert order == gold["re_sampler"][str(seed)]
        assert len(sampler) == 10 and sorted(order) == list(range(10))
        # QA pairs are shuffled inside their strided group, the groups keep their places
        assert [i % 3 for i in order] == [0] * 4 + [1] * 3 + [2] * 3
        # the reference shuffles the dataset's lists in place: a second epoch's sampler starts from the first one's order
        assert ds.group_indexs[0] == order[:4]


def test_cluster_dataset_reads_the_folder_in_sorted_order(gold):
    ds = datasets.ClusterDataset(None, CLUSTERS, 8, 32)
    assert [[int(i) for i in c] for c in ds.index_clusters] == gold["index_clusters"]
    assert len(ds) == 20 and [len(c) for c in ds.index_clusters] == [4, 7, 9]
    first_of_b = json.loads(open(os.path.join(CLUSTERS, "cluster_b.txt")).readline())
    assert ds.data[4] == first_of_b
    kept = datasets.ClusterDataset(None, CLUSTERS, 8, 32, filter=True)
    want = [sum(1 for line in open(os.path.join(CLUSTERS, f)) if ds.filter_sample(json.loads(line)))
            for f in sorted(os.listdir(CLUSTERS))]
    assert [len(c) for c in kept.index_clusters] == want and 0 < len(kept) < len(ds)


@pytest.mark.parametrize("batch_size", [4, 7])
def test_cluster_sampler_gives_the_reference_order(gold, batch_size):
    assert batch_size in gold["batch_sizes"]
    ds = datasets.ClusterDataset(None, CLUSTERS, 8, 32)
    cluster_of = {int(i): c for c, members in enumerate(ds.index_clusters) for i in members}
    for seed in gold["seeds"]:
        seed_all(seed)
        sampler = datasets.ClusterSampler(ds, batch_size)
        order = list(sampler)
        assert order == gold["cluster_sampler"][f"{seed}/{batch_size}"]
        assert len(sampler) == 20 and sorted(order) == list(range(20))
        # The batches are the batch-sized slices of the cluster-by-cluster sequence (4 + 7 + 9 items), visited in a
        # shuffled order.  A slice that no cluster boundary cuts comes from one cluster -- with batch size 4 the slices
        # [0:4], [4:8], [12:16] and [16:20]; [8:12] holds the last three of the second cluster and one of the third.
        # Every slice is found again, whole, with exactly that composition.
        pre_shuffle = [c for c, members in enumerate(ds.index_clusters) for _ in members]
        want = collections.Counter(tuple(pre_shuffle[s:s + batch_size]) for s in range(0, 20, batch_size))
        got, pos = collections.Counter(), 0
        # (a short last slice may land anywhere: np.random is consumed by the shuffle of the slice starts alone, so the
        # same seed gives the order in which the slices were visited)
        starts = np.arange(0, 20, batch_size)
        np.random.seed(seed)
        np.random.shuffle(starts)
        for s in starts:
            n = min(batch_size, 20 - s)
            batch = order[pos:pos + n]
            pos += n
            got[tuple(sorted(cluster_of[i] for i in batch))] += 1
            if len(set(pre_shuffle[s:s + n])) == 1:
                assert len({cluster_of[i] for i in batch}) == 1
        assert pos == 20 and got == want
        if batch_size == 4:
            assert sum(1 for k in got.elements() if len(set(k)) == 1) == 4


def test_dataloader_over_the_samplers_yields_module_batches(tokenizer):
    from torch.utils.data import DataLoader
    seed_all(3)
    ds = datasets.ReDataset(tokenizer, TRAIN, 8, 32)
    cds = datasets.ClusterDataset(tokenizer, CLUSTERS, 8, 32)
    for data, sampler, bs, n_batches in ((ds, datasets.ReSampler(ds), 4, 3), (cds, datasets.ClusterSampler(cds, 4), 4, 5)):
        loader = DataLoader(data, batch_size=bs, sampler=sampler, collate_fn=datasets.re_collate, num_workers=0)
        batches = list(loader)
        assert len(batches) == n_batches
        order = list(sampler)
        for b, batch in enumerate(batches):
            assert set(batch) == {"input_ids_q", "input_mask_q", "input_ids_c", "input_mask_c"}
            idx = order[b * bs:(b + 1) * bs]
            for side, limit in (("q", 8), ("c", 24)):
                ids, mask = batch[f"input_ids_{side}"], batch[f"input_mask_{side}"]
                assert ids.dtype == torch.int64 and mask.dtype == torch.bool and ids.shape == mask.shape
                assert ids.shape[0] == len(idx) and ids.shape[1] <= limit
                lens = mask.sum(1)
                # right-padded: the mask is a prefix of ones, the ids past it are the pad id 0
                assert all(mask[r, :lens[r]].all() and not mask[r, lens[r]:].any() and not ids[r, lens[r]:].any()
                           for r in range(len(idx)))
                assert int(lens.max()) == ids.shape[1] and (ids[:, 0] == tokenizer.cls_token_id).all()
                for r, i in enumerate(idx):
                    assert torch.equal(ids[r, :lens[r]], data[i][f"input_ids_{side}"])
    # truncation as ReDataset: the paragraphs of the inputs are longer than 24 tokens somewhere
    assert max(cds[i]["input_ids_c"].numel() for i in range(len(cds))) == 24
