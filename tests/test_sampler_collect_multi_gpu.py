"""proqa_sampler_collect_multi_device (IndexFlatIP.collect_labeled_multi_device): the sampler's collect with a question
dimension.  The yardstick is the single entry, question by question: rows, labels and records of the multi call must be
its bits.  The shapes sit where a wave (64 threads) or a block (256) could hold rows of two questions or run ragged:
k x pieces-per-row is 80 / 160 / 1120 / 2240 threads per question, a multiple of neither."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS = 1000
EINVAL = -1     # PROQA_EINVAL of include/proqa_hip.h
HEADS = [0, 7, 64]          # none, more than k = 5, the record's cap


@pytest.fixture(scope="module")
def indexes(gpu_device):
    """(fp16 index of 1000 integer rows, exact-float32 index of 1000 rows)"""
    from proqa_amd.index import IndexFlatIP
    rng = np.random.default_rng(2201)
    x16 = rng.integers(-4, 5, (N_ROWS, 128)).astype(np.float16)
    x32 = (rng.integers(-4, 5, (N_ROWS, 128)) * (1 + 2.0 ** -14)).astype(np.float32)     # fp16 cannot hold these
    out = {}
    for name, x in (("f16", x16), ("f32", x32)):
        index = IndexFlatIP(128)
        index.add(x)
        out[name] = index
    assert out["f32"].exact_f32 and not out["f16"].exact_f32
    return out


def _ids(rng, nq, k, lo=0):
    """[nq, k] ids of rows lo .. lo + N_ROWS, every question with a -1 and an id past the index when k allows"""
    ids = np.stack([rng.permutation(N_ROWS)[:k] for _ in range(nq)]).astype(np.int64).reshape(nq, k) + lo
    if k >= 5:
        ids[:, -1] = -1
        ids[:, k // 2] = lo + N_ROWS + np.arange(nq)         # >= ntotal
    return ids


def _gold(rng, ids, counts, lo=0):
    """one buffer with a list of counts[q] ascending ids per question, about half of them ids of its result; the lists
    lie one after another in a shuffled order, so that `begin` is not ascending; -> (buffer, begin, count)"""
    lists = []
    for q, n in enumerate(counts):
        mine = np.unique(ids[q][(ids[q] >= lo) & (ids[q] < lo + N_ROWS)])
        take = rng.permutation(mine)[:(n + 1) // 2]
        rest = np.setdiff1d(np.arange(lo, lo + 2 * N_ROWS), take)
        lists.append(np.sort(np.concatenate([take, rng.permutation(rest)[:n - len(take)]])).astype(np.int64))
    order = rng.permutation(len(counts))
    begin, at = [0] * len(counts), 0
    for q in order:
        begin[q] = at
        at += len(lists[q])
    buf = np.concatenate([lists[q] for q in order]) if len(counts) else np.empty(0, np.int64)
    return buf.astype(np.int64), begin, [len(l) for l in lists]


def _compare(index, dev, ids, gold, begin, count, head, dtype=None, idx_offset=0):
    """the multi call against one single call per question, bit for bit; the same multi call twice"""
    import torch
    ids_t = torch.from_numpy(ids).to(dev)
    gold_t = torch.from_numpy(gold).to(dev) if gold is not None and len(gold) else None
    rows, labels, records = index.collect_labeled_multi_device(ids_t, gold_t, begin, count, head, dtype, idx_offset)
    again = index.collect_labeled_multi_device(ids_t, gold_t, begin, count, head, dtype, idx_offset)
    nq, k = ids.shape
    assert rows.dtype == (dtype or torch.float16) and tuple(rows.shape) == (nq, k, 128)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (nq, k)
    assert records.dtype == torch.int64 and tuple(records.shape) == (nq, 2 + head)
    for q in range(nq):
        mine = gold_t[begin[q]:begin[q] + count[q]] if count[q] else None
        want = index.collect_labeled_device(ids_t[q], mine, head, dtype, idx_offset)
        for name, a, b in zip(("rows", "labels", "record"), (rows[q], labels[q], records[q]), want):
            assert torch.equal(a.contiguous().view(torch.uint8), b.view(torch.uint8)), (name, q)
    for a, b in zip((rows, labels, records), again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    return labels, records


@pytest.mark.parametrize("nq", [1, 3, 9])
@pytest.mark.parametrize("out", ["float16", "float32"])
@pytest.mark.parametrize("k", [5, 70])
def test_equals_the_single_entry_question_by_question(indexes, gpu_device, k, out, nq):
    """lists of 0 .. 40 ids, the middle question's list empty, one question's list ending the buffer, ids with -1 and
    ids >= ntotal, head = 0, > k (at k = 5) and 64"""
    import torch
    rng = np.random.default_rng(100 * k + nq)
    ids = _ids(rng, nq, k)
    counts = [int(c) for c in rng.integers(1, 41, nq)]
    if nq > 1:
        counts[nq // 2] = 0
    gold, begin, count = _gold(rng, ids, counts)
    assert max(b + c for b, c in zip(begin, count)) == len(gold)          # a list ends the buffer
    for head in HEADS:
        labels, records = _compare(indexes["f16"], gpu_device, ids, gold, begin, count, head, getattr(torch, out))
        assert records[:, 0].tolist() == [k - 2] * nq                     # all but the -1 and the id past the index
        assert records[:, 1].tolist() == labels.sum(dim=1).tolist()
        if nq > 1:
            assert records[nq // 2, 1].item() == 0 and records[:, 1].sum().item() > 0


@pytest.mark.parametrize("nq", [64, 65, 130])
def test_more_questions_than_one_launch_takes(indexes, gpu_device, nq):
    """the bounds go by value, 64 questions a launch: one launch exactly, one question more, and three launches"""
    rng = np.random.default_rng(nq)
    ids = _ids(rng, nq, 5)
    gold, begin, count = _gold(rng, ids, [int(c) for c in rng.integers(0, 6, nq)])
    _, records = _compare(indexes["f16"], gpu_device, ids, gold, begin, count, 7)
    assert records[:, 1].sum().item() > 0


def test_empty_lists_everywhere_and_shared_lists(indexes, gpu_device):
    rng = np.random.default_rng(3)
    ids = _ids(rng, 3, 70)
    gold, begin, count = _gold(rng, ids, [9, 9, 9])
    for buf in (None, gold):           # no buffer at all; a buffer nobody reads
        _, records = _compare(indexes["f16"], gpu_device, ids, buf, [0, 0, 0], [0, 0, 0], 5)
        assert records[:, 1].tolist() == [0, 0, 0]
    # the same question three times: three results, one list
    same = np.repeat(ids[:1], 3, axis=0)
    _, records = _compare(indexes["f16"], gpu_device, same, gold, [begin[0]] * 3, [count[0]] * 3, 5)
    assert records[0, 1].item() >= 5 and records[:, 1].tolist() == [records[0, 1].item()] * 3      # _gold took 5 of its ids
    # one question that owns the whole buffer
    whole = np.unique(gold)
    _compare(indexes["f16"], gpu_device, ids[:1], whole, [0], [len(whole)], 5)


def test_k_zero_writes_the_records_only(indexes, gpu_device):
    import torch
    ids = torch.empty((3, 0), dtype=torch.int64, device=gpu_device)
    gold = torch.arange(10, device=gpu_device)
    for head in (0, 4):
        rows, labels, records = indexes["f16"].collect_labeled_multi_device(ids, gold, [0, 3, 10], [3, 7, 0], head)
        assert tuple(rows.shape) == (3, 0, 128) and tuple(labels.shape) == (3, 0)
        assert records.tolist() == [[0, 0] + [-1] * head] * 3
    rows, labels, records = indexes["f16"].collect_labeled_multi_device(ids[:0], gold, [], [], 4)
    assert tuple(rows.shape) == (0, 0, 128) and tuple(records.shape) == (0, 6)


def test_ids_of_a_shard(indexes, gpu_device):
    """idx_offset 1000: an id below the shard that equals a gold id is a zero row with label 0, in every question"""
    rng = np.random.default_rng(5)
    ids = _ids(rng, 3, 70, lo=1000)
    ids[:, 0] = 999
    gold, begin, count = _gold(rng, ids, [12, 0, 30], lo=1000)
    gold = np.sort(np.concatenate([gold[begin[0]:begin[0] + 12], [999]])).astype(np.int64)      # question 0 alone, with 999
    lists = [gold, np.empty(0, np.int64), np.array([999, 1000 + 5], dtype=np.int64)]
    buf = np.concatenate(lists)
    labels, records = _compare(indexes["f16"], gpu_device, ids, buf, [0, 13, 13], [13, 0, 2], 6, idx_offset=1000)
    assert labels[:, 0].tolist() == [0, 0, 0] and records[:, 0].tolist() == [67, 67, 67]
    assert records[0, 1].item() >= 6          # _gold took 6 of question 0's ids


@pytest.mark.parametrize("out", ["float16", "float32"])
def test_exact_float32_index(indexes, gpu_device, out):
    import torch
    rng = np.random.default_rng(7)
    ids = _ids(rng, 3, 70)
    gold, begin, count = _gold(rng, ids, [8, 0, 21])
    _compare(indexes["f32"], gpu_device, ids, gold, begin, count, 5, getattr(torch, out))


def test_refusals_launch_nothing(indexes, gpu_device):
    """NULL ids with k > 0, head = 65 and a bad dtype are PROQA_EINVAL, and so are lists that leave the buffer; the outputs
    keep the bytes they held"""
    import torch
    from proqa_amd import _lib
    index = indexes["f16"]
    ids = torch.arange(8, device=gpu_device).reshape(2, 4)
    gold = torch.tensor([1, 5, 6], device=gpu_device)
    for bad in (ids.to(torch.int32), ids.cpu(), ids.reshape(-1)):
        with pytest.raises(ValueError):
            index.collect_labeled_multi_device(bad, gold, [0, 1], [1, 2], 2)
    for bad in (gold.to(torch.int32), gold.cpu()):
        with pytest.raises(ValueError):
            index.collect_labeled_multi_device(ids, bad, [0, 1], [1, 2], 2)
    with pytest.raises(ValueError):
        index.collect_labeled_multi_device(ids, gold, [0], [1], 2)
    for head in (-1, 65):
        with pytest.raises(_lib.ProqaError) as e:
            index.collect_labeled_multi_device(ids, gold, [0, 1], [1, 2], head)
        assert e.value.code == EINVAL
    for begin, count in (([0, 2], [1, 2]), ([-1, 0], [1, 1]), ([0, 4], [1, 0]), ([0, 0], [1, -1])):
        with pytest.raises(_lib.ProqaError) as e:
            index.collect_labeled_multi_device(ids, gold, begin, count, 2)
        assert e.value.code == EINVAL
    lib = _lib.load()
    rows = torch.full((2, 4, 128), 7, dtype=torch.float16, device=gpu_device)
    labels = torch.full((2, 4), 7, dtype=torch.int32, device=gpu_device)
    records = torch.full((2, 4), 7, dtype=torch.int64, device=gpu_device)
    torch.cuda.synchronize()
    i64x2 = ctypes.c_int64 * 2

    def call(h=index._h, ids_ptr=ids.data_ptr(), nq=2, k=4, gold_ptr=gold.data_ptr(), n_gold=3, begin=(0, 1), count=(1, 2), head=2,
             dtype=_lib.PROQA_F16, record_ptr=records.data_ptr()):
        return lib.proqa_sampler_collect_multi_device(h, ids_ptr, nq, k, 0, gold_ptr, n_gold, i64x2(*begin), i64x2(*count), head,
                                                      rows.data_ptr(), dtype, labels.data_ptr(), record_ptr, None)
    assert call(h=ctypes.c_void_p()) == EINVAL
    assert call(ids_ptr=None) == EINVAL
    assert call(head=65) == EINVAL
    assert call(dtype=99) == EINVAL
    assert call(k=-1) == EINVAL and call(nq=-1) == EINVAL
    assert call(gold_ptr=None) == EINVAL
    assert call(record_ptr=None) == EINVAL
    assert call(begin=(0, 2), count=(1, 2)) == EINVAL
    torch.cuda.synchronize()
    assert (rows == 7).all() and (labels == 7).all() and (records == 7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert records.tolist() == [[4, 1, 0, 1], [4, 2, 4, 5]] and labels.tolist() == [[0, 1, 0, 0], [0, 1, 1, 0]]
    assert call(gold_ptr=None, n_gold=0, count=(0, 0), begin=(0, 0)) == 0
    torch.cuda.synchronize()
    assert records[:, 1].tolist() == [0, 0]
