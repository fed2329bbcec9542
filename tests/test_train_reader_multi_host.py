"""train_reader.py --questions-per-pass without a GPU: the grouping rule (pass_schedule / closes_pass, next to
update_schedule), the flag's default and refusal, and the resume fingerprint's rule for the new field."""
import itertools

import pytest

from proqa_amd import train_reader
from proqa_amd.pretrain_retriever import is_update_step
from proqa_amd.train_reader import closes_pass, pass_schedule, update_schedule

N = 13          # questions of an epoch: no multiple of any G or Q below, so the epoch ends inside a window
FAILED_SETS = [(), (4,), (3, 4), (8,), (13,), (1, 2, 3, 4), (4, 8, 12, 13), (5, 6, 7), tuple(range(1, 14))]


@pytest.mark.parametrize("G,Q", list(itertools.product([1, 2, 4], [1, 2, 3, 8])))
def test_passes_are_the_windows_cut_into_pieces(G, Q):
    for first in (1, 14):               # the second epoch's batch steps go on counting
        for failed in FAILED_SETS:
            failed = [f + first - 1 for f in failed]
            passes = pass_schedule(N, G, Q, failed=failed, first=first)
            steps = [b for b in range(first, first + N) if b not in set(failed)]
            assert [b for p in passes for b in p] == steps                      # every retrieved question once, in order
            assert all(1 <= len(p) <= Q for p in passes)
            updates = set(update_schedule(first + N - 1, G, failed=failed))
            for p in passes:
                assert not any(b in updates for b in p[:-1])                    # no pass continues past an update
            for b in steps:
                if b in updates:
                    assert any(p[-1] == b for p in passes)                      # an update finds every gradient of its window
            if Q == 1:
                assert passes == [[b] for b in steps]
            if G == 1:
                assert all(len(p) == 1 for p in passes)
            # a pass is as large as the rule allows: it closes early only at an update or at the epoch's end
            for p in passes[:-1]:
                assert len(p) == Q or p[-1] in updates
            # a failed retrieval in an update slot leaves the window, and the pass, open
            for f in failed:
                if is_update_step(f, G) and f + 1 in steps and f - 1 in steps and (f - 1) not in updates and Q >= 2:
                    mine = next(p for p in passes if f - 1 in p)
                    assert len(mine) == Q or f + 1 in mine or mine[-1] in updates


def test_the_examples_of_the_documents():
    # G = 4: the update slots are the batch steps 3, 7, 11, ... ((batch_step + 1) % G == 0, the reference's rule)
    assert pass_schedule(8, 4, 3) == [[1, 2, 3], [4, 5, 6], [7], [8]]
    assert pass_schedule(8, 4, 3, failed=[5]) == [[1, 2, 3], [4, 6, 7], [8]]
    assert pass_schedule(8, 4, 8, failed=[3]) == [[1, 2, 4, 5, 6, 7], [8]]          # the failed slot leaves the window open
    assert pass_schedule(6, 4, 8) == [[1, 2, 3], [4, 5, 6]]                        # the epoch ends inside a window
    assert pass_schedule(8, 4, 3, failed=[8]) == [[1, 2, 3], [4, 5, 6], [7]]
    assert pass_schedule(3, 4, 3, first=9) == [[9, 10, 11]]
    assert pass_schedule(3, 1, 8) == [[1], [2], [3]]
    assert pass_schedule(0, 2, 2) == [] and pass_schedule(2, 2, 2, failed=[1, 2]) == []
    assert closes_pass(3, 6, 4, 3) and closes_pass(1, 7, 4, 3) and not closes_pass(2, 6, 4, 3)


def test_one_question_per_pass_is_the_smallest_case_of_the_one_loop():
    """The trainer has one loop body for every Q: at Q = 1 it must run every retrieved question as a pass of its own, at once."""
    n = 12
    for G in (1, 4):
        failed = [6]                    # inside a window at G = 4 (the update slots are 3, 7, 11)
        assert not is_update_step(6, 4)
        assert pass_schedule(n, G, 1, failed) == [[b] for b in range(1, n + 1) if b not in failed]
        assert all(closes_pass(1, b, G, 1) for b in range(1, 3 * n))
    assert "questions_per_pass" not in train_reader.reader_fingerprint_extra(_args("--questions-per-pass", "1"))


def test_update_schedule_is_unchanged():
    assert update_schedule(8, 2) == [1, 3, 5, 7]
    assert update_schedule(8, 2, failed=[3]) == [1, 5, 7]
    assert update_schedule(9, 4, failed=[1, 7]) == [3]
    assert update_schedule(5, 1, failed=[2]) == [1, 3, 4, 5]


def _args(*flags):
    return train_reader.get_args(["--matched-para-path", "m.txt", *flags])


def test_flag_default_and_refusal():
    assert _args().questions_per_pass == 1
    assert train_reader.check_args(_args("--questions-per-pass", "8")).questions_per_pass == 8
    with pytest.raises(ValueError, match="questions_per_pass"):
        train_reader.check_args(_args("--questions-per-pass", "0"))


def test_fingerprint_gains_the_field_only_when_it_is_not_one():
    from proqa_amd import checkpoint
    base = train_reader.reader_fingerprint_extra(_args())
    assert "questions_per_pass" not in base and set(base) == {"qa_drop", "shared_norm", "drop_early", "fix_para_encoder"}
    assert train_reader.reader_fingerprint_extra(_args("--questions-per-pass", "1")) == base
    three = train_reader.reader_fingerprint_extra(_args("--questions-per-pass", "3"))
    assert three == dict(base, questions_per_pass=3)

    def fp(*flags):
        a = _args(*flags)
        return checkpoint.fingerprint("train_reader.py", a, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                                      extra=train_reader.reader_fingerprint_extra(a))
    assert list(fp()) == list(fp("--questions-per-pass", "1")) and "questions_per_pass" not in fp()
    checkpoint.check_fingerprint(fp(), fp())                                        # state files of today keep resuming
    checkpoint.check_fingerprint(fp("--questions-per-pass", "3"), fp("--questions-per-pass", "3"))
    train_reader.check_field_default_1(fp(), "questions_per_pass", 1)
    train_reader.check_field_default_1(fp("--questions-per-pass", "3"), "questions_per_pass", 3)
    with pytest.raises(SystemExit, match="'questions_per_pass' is 1 now, was 3"):
        train_reader.check_field_default_1(fp("--questions-per-pass", "3"), "questions_per_pass", 1)
    with pytest.raises(SystemExit, match="'questions_per_pass' is 3 now, was 1"):
        train_reader.check_field_default_1(fp(), "questions_per_pass", 3)
    with pytest.raises(SystemExit, match="'questions_per_pass' is 2 now, was 3"):
        checkpoint.check_fingerprint(fp("--questions-per-pass", "3"), fp("--questions-per-pass", "2"))
