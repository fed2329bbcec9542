"""The pair loop of the int8 nomination scan (mips_filter_i8: per-pair LDS-DMA issue from running addresses, clamped only in a
chunk's last pair; no fragment re-read behind a pair's last unit; a scalar running pointer to the block constants) must stay
invisible: ids and score bits are the fp16 scan's, the rows it nominates are the rows the scan nominated before the loop was
rewritten (tests/golden/filter_i8_tiles_nominated.json: `last_stats()["nominated"]` recorded from that library for the same
inputs; the nominee set of a round depends on the thresholds and the rows alone), and no round falls back on Gaussian rows.

Replaces the same call site as every search test: retrieval/eval_retrieval.py:98-104 of the reference.

Shapes (seeded N(0,1) fp16 rows; mode "always" lets small shards and small batches take the int8 rounds):
  queries  257 (the smallest batch with two query blocks per wave: one 512-query tile, all padding but 257 queries, so it has
           waves that only stream), 300, 513 (two tiles)
  rows     512 (the smallest index "always" accepts: most chunks are empty), 4224 = 33 x 128, and 70001: chunks of whole
           256-row pairs and of a trailing one-stage pair, and a last chunk that ends in a partial 32-row unit (the tail clip
           of the records and the clamped DMA); 200000 rows searched at idx_offset != 0; 400000 rows: chunks of 896 rows,
           three whole pairs (both pair buffers refilled) and a one-stage pair
  k        80 and 1
and a 32-query (row-split) and a 200-query search on 70001 rows: the one-query-block launches."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = (512, 4224, 70001)
QUERIES = (257, 300, 513)
KS = (80, 1)
OFFSET_CASE = (200000, 300, 80, 1234567)     # rows, queries, k, idx_offset
LONG_CHUNKS_CASE = (400000, 300, 80, 0)
SMALL_BATCHES = (32, 200)                    # on 70001 rows, k = 80
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_i8_tiles_nominated.json")

_cache = {}


def _data():
    """the corpus (every case searches a prefix of it) and the queries, computed once"""
    if "data" not in _cache:
        rng = np.random.default_rng(1701)
        xb = rng.standard_normal((LONG_CHUNKS_CASE[0], 128), dtype=np.float32).astype(np.float16)
        xq = rng.standard_normal((max(QUERIES), 128), dtype=np.float32).astype(np.float16)
        _cache["data"] = (xb, xq)
    return _cache["data"]


def _indexes(rows):
    """(fp16-scan index, int8-scan index) over the first `rows` rows, built once per size"""
    from proqa_amd.index import IndexFlatIP
    if ("ix", rows) not in _cache:
        pair = []
        for mode in ("off", "always"):
            ix = IndexFlatIP(128)
            ix.configure_nomination(mode)
            ix.add(_data()[0][:rows])
            pair.append(ix)
        _cache[("ix", rows)] = pair
    return _cache[("ix", rows)]


def search_both(rows, nq, k, idx_offset=0):
    """((D, I, stats) of the fp16 scan, the same of the int8 scan) for the first nq queries on the first `rows` rows"""
    import torch
    tq = torch.from_numpy(_data()[1][:nq]).cuda()
    out = []
    for ix in _indexes(rows):
        D, I = ix.search_device(tq, k, idx_offset=idx_offset)
        out.append((D.cpu().numpy(), I.cpu().numpy(), ix.last_stats()))
    return out


def case_key(rows, nq, k, idx_offset=0):
    return f"rows={rows} nq={nq} k={k} offset={idx_offset}"


def _check(rows, nq, k, idx_offset=0):
    (D0, I0, st0), (D1, I1, st1) = search_both(rows, nq, k, idx_offset)
    golden = json.load(open(GOLDEN))
    print(f"{case_key(rows, nq, k, idx_offset)}: nominated {st1['nominated']} (recorded {golden[case_key(rows, nq, k, idx_offset)]}), "
          f"rounds {st1['rounds']}, fallback rounds {st1['fallback_rounds']}")
    assert st1["nomination"] and not st0["nomination"]
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1.view(np.int32), D0.view(np.int32))
    assert st1["fallback_rounds"] == 0, st1
    assert st1["nominated"] == golden[case_key(rows, nq, k, idx_offset)], st1


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("nq", QUERIES)
@pytest.mark.parametrize("rows", ROWS)
def test_two_block_scan_is_the_fp16_scan_bit_for_bit(gpu_device, rows, nq, k):
    _check(rows, nq, k)


def test_two_block_scan_at_an_index_offset(gpu_device):
    rows, nq, k, off = OFFSET_CASE
    _check(rows, nq, k, off)


def test_two_block_scan_over_chunks_of_several_pairs(gpu_device):
    _check(*LONG_CHUNKS_CASE)


@pytest.mark.parametrize("nq", SMALL_BATCHES)
def test_one_block_launches_of_small_batches(gpu_device, nq):
    _check(70001, nq, 80)
