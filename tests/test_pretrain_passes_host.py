"""The host side of pretrain_retriever.py --micro-batches-per-pass: the float64 oracle of the block-diagonal objective
(tests/inbatch_blocks_oracle.py), the pass schedule against the reference's update rule, the flag and the resume
fingerprint, and the argument refusals of the two entry points.  No GPU."""
import ctypes

import pytest
import torch

import inbatch_blocks_oracle as oracle
import test_inbatch_blocks_gpu as G
from proqa_amd import checkpoint
from proqa_amd import pretrain_retriever as cmd
from proqa_amd.config import get_args


# ---- the oracle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["1", "33", "ragged", "6x3"])
def test_closed_form_equals_autograd(name):
    q, c, sizes, ref = G.case(name)
    closed = oracle.closed_form(q, c, sizes, G.grad_in_of(sizes))
    for k in ("loss", "dq", "dc"):
        assert float((closed[k] - ref[k]).abs().max()) <= 1e-12 * max(1.0, float(ref[k].abs().max())), k


def test_the_oracle_is_per_block_cross_entropy():
    """every block alone through tests/train_oracle.py's single-rectangle oracle, weighted by its grad_in; nothing crosses
    a block's border"""
    import train_oracle
    q, c, sizes, ref = G.case("ragged")
    o, g = oracle.offsets_of(sizes), G.grad_in_of(sizes)
    for m in range(len(sizes)):
        qm, cm = q[o[m]:o[m + 1]], c[o[m]:o[m + 1]]
        single = train_oracle.inbatch_loss_grad(qm, cm, None, grad_in=g[m])
        assert torch.allclose(single["dq"], ref["dq"][o[m]:o[m + 1]], rtol=0, atol=1e-13)
        assert torch.allclose(single["dc"], ref["dc"][o[m]:o[m + 1]], rtol=0, atol=1e-13)
        assert abs(float(train_oracle.inbatch_loss(qm.double(), cm.double())) - float(ref["loss"][m])) <= 1e-13
    # another block's rows do not matter
    q2 = q.clone()
    q2[o[1]:o[2]] = 7.0
    moved = oracle.evaluate(q2, c, sizes, g)
    assert torch.equal(moved["dq"][o[2]:], ref["dq"][o[2]:]) and torch.equal(moved["dc"][:o[1]], ref["dc"][:o[1]])


def test_storage_mode_rounds_the_final_gradients_to_fp16():
    q, c, sizes, ref = G.case("80x3")
    got = oracle.evaluate(q, c, sizes, G.grad_in_of(sizes), dtype=torch.float32, storage="fp16")
    assert got["dq"].dtype == torch.float32 and torch.equal(got["dq"], got["dq"].half().float())
    assert 0 < oracle.rel_err(got["dq"], ref["dq"]) < 1e-3


def test_reference_error_table_is_reproduced():
    """the GPU test's bounds are four times these numbers; they are measured here, on the CPU"""
    table = G.measure_reference_error()
    print(table)
    assert set(table) == set(G.REFERENCE_ERROR)
    for k, v in table.items():
        assert abs(v - G.REFERENCE_ERROR[k]) <= 0.1 * G.REFERENCE_ERROR[k], (k, v)


# ---- the schedule ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G_", [1, 2, 4, 8])
@pytest.mark.parametrize("M", [1, 2, 3, 4, 8, 64])
@pytest.mark.parametrize("n,first", [(1, 1), (7, 1), (21, 1), (13, 22), (40, 5)])
def test_pass_schedule_against_update_schedule(G_, M, n, first):
    passes = cmd.pass_schedule(n, G_, M, first=first)
    steps = list(range(first, first + n))
    assert [b for p in passes for b in p] == steps                       # concatenated: every micro-batch once, in order
    assert all(1 <= len(p) <= M for p in passes)
    updates = set(cmd.update_schedule(first + n, G_))
    for p in passes:
        assert not any(b in updates for b in p[:-1])                     # inside one window: an update only ends a pass
    # a pass is short only at an update step or at the epoch's end
    for p in passes[:-1]:
        assert len(p) == M or p[-1] in updates
    if G_ == 1 or M == 1:
        assert passes == [[b] for b in steps]
    # the update steps are the reference's, and each closes a pass
    ends = {p[-1] for p in passes}
    assert all(b in ends for b in steps if cmd.is_update_step(b, G_))


def test_pass_schedule_examples():
    # G = 8: the first update follows SEVEN micro-batches, so the first window's passes hold seven
    assert cmd.pass_schedule(20, 8, 8) == [[1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 14, 15], [16, 17, 18, 19, 20]]
    assert cmd.pass_schedule(20, 8, 4) == [[1, 2, 3, 4], [5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [16, 17, 18, 19], [20]]
    assert cmd.update_schedule(20, 8) == [7, 15]
    # an epoch's short tail forms the last pass; the next epoch goes on inside the same window
    assert cmd.pass_schedule(5, 4, 4) == [[1, 2, 3], [4, 5]]
    assert cmd.pass_schedule(5, 4, 4, first=6) == [[6, 7], [8, 9, 10]]
    assert cmd.pass_schedule(0, 4, 4) == []


# ---- the flag and the fingerprint ---------------------------------------------------------------------------------------------

def _args(*extra):
    return get_args(["--train_file", "data/nq-train.txt", "--predict_file", "dev.txt", *extra])


def test_flag_default_and_refusal():
    assert cmd.check_args(_args()).micro_batches_per_pass == 1
    assert cmd.check_args(_args("--micro-batches-per-pass", "8")).micro_batches_per_pass == 8
    for bad in ("0", "-3"):
        with pytest.raises(SystemExit, match="micro-batches-per-pass"):
            cmd.check_args(_args("--micro-batches-per-pass", bad))


def test_fingerprint_gains_the_field_only_when_it_is_not_1():
    def fp(*extra):
        args = cmd.check_args(_args(*extra))
        return checkpoint.fingerprint("pretrain_retriever.py", args, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                                      extra=cmd.fingerprint_extra(args))
    plain, one, four = fp(), fp("--micro-batches-per-pass", "1"), fp("--micro-batches-per-pass", "4")
    assert plain == one and "micro_batches_per_pass" not in plain
    assert four == dict(plain, micro_batches_per_pass=4)
    # a state file without the field (written before the flag existed, or at 1) still resumes at 1 ...
    cmd.check_micro_batches_per_pass(plain, 1)
    checkpoint.check_fingerprint(plain, one)
    # ... and is refused at any other value, as a state written at 4 is at 2 or at 1
    for saved, now in ((plain, 2), (four, 2), (four, 1)):
        with pytest.raises(SystemExit, match="micro_batches_per_pass"):
            cmd.check_micro_batches_per_pass(saved, now)
    cmd.check_micro_batches_per_pass(four, 4)
    checkpoint.check_fingerprint(four, four)


# ---- argument refusals of the entry points ------------------------------------------------------------------------------------

def test_abi_refuses_bad_geometry_without_a_gpu():
    from proqa_amd import _lib
    lib = _lib.load()
    ptr = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before the device is touched

    def offsets(*o):
        return (ctypes.c_int32 * len(o))(*o)

    def forward(offs, M, n, dim=128):
        return lib.proqa_inbatch_loss_blocks_f16(ptr, ptr, offs, M, n, dim, ptr, ptr, ptr, None)

    def backward(offs, M, n, dim=128):
        return lib.proqa_inbatch_loss_blocks_grad_f16(ptr, ptr, offs, M, n, dim, ptr, ptr, ptr, ptr, None)

    many = offsets(*range(66))
    for call in (forward, backward):
        for args, word in (((offsets(0), 0, 0), b"n_blocks=0"),                       # M = 0
                           ((many, 65, 65), b"n_blocks=65"),                          # M = 65
                           ((offsets(0, 8, 8, 20), 3, 20), b"block 1 is [8, 8)"),     # an empty block
                           ((offsets(0, 8, 4, 20), 3, 20), b"block 1 is [8, 4)"),     # descending
                           ((offsets(0, 8, 16), 2, 20), b"from 0 to n=20"),           # offsets that do not end at n
                           ((offsets(1, 8, 20), 2, 20), b"from 0 to n=20"),           # nor start at 0
                           ((offsets(0, 8, 20), 2, 20, 64), b"dim=64"),               # dim != 128
                           ((offsets(0, 1 << 24, (1 << 24) + 1), 2, (1 << 24) + 1), b"2^24"),
                           ((None, 2, 20), b"NULL block_offsets")):
            assert call(*args) == -1, args
            assert word in lib.proqa_last_error(), (args, lib.proqa_last_error())


def test_block_offsets_helper():
    from proqa_amd.inbatch import MAX_BLOCKS, block_offsets
    assert list(block_offsets([3, 1, 5], 9)) == [0, 3, 4, 9]
    assert list(block_offsets(torch.tensor([2, 2]), 4)) == [0, 2, 4]
    for sizes, n in (([], 0), ([1] * (MAX_BLOCKS + 1), MAX_BLOCKS + 1), ([3, 0], 3), ([3, 3], 7)):
        with pytest.raises(ValueError):
            block_offsets(sizes, n)
