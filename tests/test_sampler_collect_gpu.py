"""proqa_sampler_collect_device (IndexFlatIP.collect_labeled_device): the collect step of the reader's online sampler in
one launch.  Rows bit-equal to reconstruct_batch_device, labels = numpy.isin(ids, gold) and live, the record as
include/proqa_hip.h defines it, and identical outputs from two calls."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SMALL, N_LARGE = 600, 9000
KS = [1, 5, 15, 16, 17, 255, 256, 257]
N_GOLDS = [0, 1, 2, 3, 7, 8, 9, 1000]
EINVAL = -1     # PROQA_EINVAL of include/proqa_hip.h


@pytest.fixture(scope="module")
def indexes(gpu_device):
    """(fp16 index of 600 integer rows, exact-float32 index of 600 rows, fp16 index of 9000 rows) with their host rows"""
    from proqa_amd.index import IndexFlatIP
    rng = np.random.default_rng(1501)
    x16 = rng.integers(-4, 5, (N_SMALL, 128)).astype(np.float16)
    x32 = (rng.integers(-4, 5, (N_SMALL, 128)) * (1 + 2.0 ** -14)).astype(np.float32)     # fp16 cannot hold these
    xl = rng.integers(-4, 5, (N_LARGE, 128)).astype(np.float16)
    out = {}
    for name, x in (("f16", x16), ("f32", x32), ("large", xl)):
        index = IndexFlatIP(128)
        index.add(x)
        out[name] = (index, x)
    assert out["f32"][0].exact_f32 and not out["f16"][0].exact_f32
    return out


def _expect(ids, gold, n, head, idx_offset=0):
    live = (ids >= idx_offset) & (ids < idx_offset + n)
    labels = (np.isin(ids, gold) & live).astype(np.int32)
    record = np.full(2 + head, -1, dtype=np.int64)
    record[0], record[1] = live.sum(), labels.sum()
    m = min(head, len(ids))
    record[2:2 + m] = ids[:m]
    return labels, record


def _check(index, dev, ids, gold, head, dtype=None, idx_offset=0):
    import torch
    ids_t = torch.from_numpy(ids).to(dev)
    gold_t = torch.from_numpy(gold).to(dev) if gold is not None else None
    rows, labels, record = index.collect_labeled_device(ids_t, gold_t, head, dtype, idx_offset)
    again = index.collect_labeled_device(ids_t, gold_t, head, dtype, idx_offset)
    want_rows = index.reconstruct_batch_device(ids_t, dtype, idx_offset)
    want_labels, want_record = _expect(ids, gold if gold is not None else np.empty(0, np.int64), index.ntotal, head, idx_offset)
    assert rows.dtype == (dtype or torch.float16) and tuple(rows.shape) == (len(ids), 128)
    assert labels.dtype == torch.int32 and record.dtype == torch.int64 and tuple(record.shape) == (2 + head,)
    assert torch.equal(rows.view(torch.uint8), want_rows.view(torch.uint8))       # bit for bit
    np.testing.assert_array_equal(labels.cpu().numpy(), want_labels)
    np.testing.assert_array_equal(record.cpu().numpy(), want_record)
    for a, b in zip((rows, labels, record), again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    return labels, record


def _gold_list(rng, ids, n_gold, lo, hi):
    """n_gold strictly ascending ids from [lo, hi), about half of them ids of the result"""
    from_result = np.unique(ids[(ids >= lo) & (ids < hi)])
    take = rng.permutation(from_result)[:(n_gold + 1) // 2]
    rest = np.setdiff1d(np.arange(lo, hi), take)
    gold = np.concatenate([take, rng.permutation(rest)[:n_gold - len(take)]])
    assert len(gold) == n_gold or hi - lo < n_gold
    return np.sort(gold).astype(np.int64)


@pytest.mark.parametrize("k", KS)
def test_rows_labels_and_record(indexes, gpu_device, k):
    """every head in {0, 1, 5, k (capped at the record's 64)} x every gold length, ids with a tail of -1"""
    rng = np.random.default_rng(k)
    index, _ = indexes["f16"]
    ids = rng.permutation(N_SMALL)[:k].astype(np.int64) if k <= N_SMALL else rng.integers(0, N_SMALL, k)
    if k >= 5:
        ids[-(k // 5):] = -1
    for head in sorted({0, 1, 5, min(k, 64)}):
        for n_gold in N_GOLDS:
            gold = _gold_list(rng, ids, n_gold, 0, 2000)          # ids >= 600 never occur in the result
            labels, _ = _check(index, gpu_device, ids, gold if n_gold else None, head)
            if n_gold == 1000 and k >= 15:
                assert labels.sum().item() > 0


def test_k_5000_over_9000_rows(indexes, gpu_device):
    import torch
    rng = np.random.default_rng(5000)
    index, x = indexes["large"]
    ids = rng.permutation(N_LARGE)[:5000].astype(np.int64)
    ids[4990:] = -1
    gold = _gold_list(rng, ids, 1000, 0, N_LARGE)
    labels, record = _check(index, gpu_device, ids, gold, 5)
    assert record[0].item() == 4990 and record[1].item() == labels.sum().item() > 0
    _check(index, gpu_device, ids, gold, 64, torch.float32)


def test_gold_lists_at_the_edges(indexes, gpu_device):
    rng = np.random.default_rng(9)
    index, _ = indexes["f16"]
    ids = rng.permutation(N_SMALL)[:257].astype(np.int64)
    smallest_largest = np.array([ids.min(), ids.max()], dtype=np.int64)
    _, record = _check(index, gpu_device, ids, smallest_largest, 5)
    assert record[1].item() == 2
    disjoint = np.setdiff1d(np.arange(N_SMALL), ids).astype(np.int64)
    _, record = _check(index, gpu_device, ids, disjoint, 5)
    assert record[1].item() == 0
    _, record = _check(index, gpu_device, ids, np.sort(ids), 5)
    assert record[1].item() == 257 == record[0].item()


def test_head_longer_than_k_and_k_zero(indexes, gpu_device):
    import torch
    index, _ = indexes["f16"]
    _, record = _check(index, gpu_device, np.array([7, 3, 599], dtype=np.int64), np.array([3], dtype=np.int64), 5)
    assert record.tolist() == [3, 1, 7, 3, 599, -1, -1]
    for head in (0, 4):
        rows, labels, record = index.collect_labeled_device(torch.empty(0, dtype=torch.int64, device=gpu_device), None, head)
        assert tuple(rows.shape) == (0, 128) and labels.numel() == 0
        assert record.tolist() == [0, 0] + [-1] * head


def test_gold_id_outside_the_shard_is_not_labelled(indexes, gpu_device):
    """a shard's global ids: idx_offset 1000; id 999 lies below the shard and equals a gold id -> zero row, label 0"""
    index, _ = indexes["f16"]
    ids = np.array([1000, 999, 1599, 1600, 1234, -1], dtype=np.int64)
    gold = np.array([999, 1000, 1600], dtype=np.int64)
    labels, record = _check(index, gpu_device, ids, gold, 6, idx_offset=1000)
    assert labels.tolist() == [1, 0, 0, 0, 0, 0] and record[:2].tolist() == [3, 1]


@pytest.mark.parametrize("which", ["f16", "f32"])
def test_both_output_types_on_both_kinds_of_index(indexes, gpu_device, which):
    import torch
    rng = np.random.default_rng(77)
    index, x = indexes[which]
    ids = rng.integers(-1, N_SMALL, 300).astype(np.int64)
    gold = _gold_list(rng, ids, 9, 0, N_SMALL)
    for dtype in (torch.float16, torch.float32):
        _check(index, gpu_device, ids, gold, 5, dtype)
    if which == "f32":      # the float32 copies themselves
        rows, _, _ = index.collect_labeled_device(torch.from_numpy(ids).to(gpu_device), None, 0, torch.float32)
        want = np.where((ids >= 0)[:, None], x[ids.clip(0)], 0).astype(np.float32)
        np.testing.assert_array_equal(rows.cpu().numpy(), want)


def test_refusals(indexes, gpu_device):
    import torch
    from proqa_amd import _lib
    index, _ = indexes["f16"]
    ids = torch.arange(4, device=gpu_device)
    gold = torch.tensor([1], device=gpu_device)
    for bad in (ids.to(torch.int32), ids.cpu()):
        with pytest.raises(ValueError):
            index.collect_labeled_device(bad, gold, 2)
    for bad in (gold.to(torch.int32), gold.cpu()):
        with pytest.raises(ValueError):
            index.collect_labeled_device(ids, bad, 2)
    for head in (-1, 65):
        with pytest.raises(_lib.ProqaError) as e:
            index.collect_labeled_device(ids, gold, head)
        assert e.value.code == EINVAL
    # the remaining PROQA_EINVAL cases cannot be reached through the wrapper's own checks: the bound symbol itself
    lib = _lib.load()
    rows = torch.empty((4, 128), dtype=torch.float16, device=gpu_device)
    labels = torch.empty(4, dtype=torch.int32, device=gpu_device)
    record = torch.empty(4, dtype=torch.int64, device=gpu_device)
    torch.cuda.synchronize()

    def call(h=index._h, k=4, gold_ptr=gold.data_ptr(), n_gold=1, head=2, dtype=_lib.PROQA_F16):
        return lib.proqa_sampler_collect_device(h, ids.data_ptr(), k, 0, gold_ptr, n_gold, head, rows.data_ptr(), dtype,
                                                labels.data_ptr(), record.data_ptr(), None)
    assert call() == 0
    torch.cuda.synchronize()
    assert record.tolist() == [4, 1, 0, 1]
    assert call(h=ctypes.c_void_p()) == EINVAL
    assert call(k=-1) == EINVAL
    assert call(gold_ptr=None, n_gold=1) == EINVAL
    assert call(dtype=99) == EINVAL
    assert call(gold_ptr=None, n_gold=0) == 0
    torch.cuda.synchronize()
