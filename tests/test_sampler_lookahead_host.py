"""train_reader.py --sampler-lookahead without a GPU: the grouping rule, the refusal, the resume fingerprint and the
declaration of the new entry point."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("first", [1, 6, 17])
@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("G", [1, 2, 4])
def test_groups_end_at_update_slots_at_w_and_with_the_epoch(G, W, first):
    from proqa_amd.pretrain_retriever import is_update_step
    from proqa_amd.train_reader import retrieval_groups
    for n in (0, 1, 7, 8, 13):
        groups = retrieval_groups(n, G, W, first=first)
        assert [b for g in groups for b in g] == list(range(first, first + n))
        for i, g in enumerate(groups):
            assert 1 <= len(g) <= W
            assert not any(is_update_step(b, G) for b in g[:-1])          # no group crosses an update slot
            # a group ends for one of the three reasons, and for no other
            assert is_update_step(g[-1], G) or len(g) == W or i == len(groups) - 1
    if W == 1 or G == 1:
        assert all(len(g) == 1 for g in retrieval_groups(13, G, W, first=first))


def test_groups_by_hand():
    from proqa_amd.train_reader import retrieval_groups
    # G = 4: update slots at the batch steps 3, 7, 11, 15, ...
    assert retrieval_groups(8, 4, 4) == [[1, 2, 3], [4, 5, 6, 7], [8]]
    assert retrieval_groups(8, 4, 3) == [[1, 2, 3], [4, 5, 6], [7], [8]]
    assert retrieval_groups(8, 4, 8, first=9) == [[9, 10, 11], [12, 13, 14, 15], [16]]
    assert retrieval_groups(5, 2, 8) == [[1], [2, 3], [4, 5]]
    assert retrieval_groups(3, 1, 8) == [[1], [2], [3]]
    assert retrieval_groups(0, 4, 4) == []


def test_the_loop_s_rule_is_the_schedule_s():
    """group_length, which the loop hands to the sampler, asked at every group's first step, gives the schedule's groups"""
    from proqa_amd.train_reader import group_length, retrieval_groups
    for G in (1, 2, 4):
        for W in (2, 3, 8):
            for g in retrieval_groups(20, G, W, first=5)[:-1]:
                assert group_length(g[0], G, W) == len(g)


def _args(*flags):
    from proqa_amd import train_reader
    return train_reader.build_parser().parse_args(["--raw-train-data", "t", "--raw-eval-data", "d", "--matched-para-path", "m",
                                                   *flags])


def test_check_args_refuses_a_lookahead_below_one():
    from proqa_amd import train_reader
    assert _args().sampler_lookahead == 1
    assert train_reader.check_args(_args("--sampler-lookahead", "4")).sampler_lookahead == 4
    for bad in ("0", "-2"):
        with pytest.raises(ValueError, match="sampler_lookahead"):
            train_reader.check_args(_args("--sampler-lookahead", bad))


def test_fingerprint_gains_the_field_only_when_it_is_not_one():
    from proqa_amd import train_reader
    plain = train_reader.reader_fingerprint_extra(_args())
    assert "sampler_lookahead" not in plain
    assert train_reader.reader_fingerprint_extra(_args("--sampler-lookahead", "1")) == plain
    assert train_reader.reader_fingerprint_extra(_args("--sampler-lookahead", "4")) == dict(plain, sampler_lookahead=4)
    train_reader.check_field_default_1(plain, "sampler_lookahead", 1)
    train_reader.check_field_default_1({"sampler_lookahead": 4}, "sampler_lookahead", 4)
    with pytest.raises(SystemExit, match="field 'sampler_lookahead' is 2 now, was 4 when the state was saved"):
        train_reader.check_field_default_1({"sampler_lookahead": 4}, "sampler_lookahead", 2)
    with pytest.raises(SystemExit, match="field 'sampler_lookahead' is 4 now, was 1 when the state was saved"):
        train_reader.check_field_default_1(plain, "sampler_lookahead", 4)


def test_the_entry_point_is_declared_and_the_abi_version_stays():
    from proqa_amd import _lib
    header = open(os.path.join(ROOT, "include", "proqa_hip.h")).read()
    assert re.search(r"\bint proqa_sampler_collect_multi_device\(proqa_index\* idx,", header)
    assert re.search(r"#define\s+PROQA_ABI_VERSION\s+7\b", header)
    restype, argtypes = _lib.SIGNATURES["proqa_sampler_collect_multi_device"]
    declared = header[header.index("int proqa_sampler_collect_multi_device("):]
    declared = declared[:declared.index(");")]
    assert len(argtypes) == declared.count(",") + 1 == 15
    lib = _lib.load()
    assert lib.proqa_abi_version() == 7
    assert lib.proqa_sampler_collect_multi_device.argtypes == argtypes
