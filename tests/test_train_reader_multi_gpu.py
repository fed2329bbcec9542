"""train_reader.py --questions-per-pass end to end on the tiny model and files of tests/test_train_reader_gpu.py.

G = 4 (update slots at the batch steps 3, 7, 11), dropout 0, --deterministic, seed 11: the question without an answer
anywhere is the 5th of the first epoch, a failed retrieval INSIDE the second window (no update slot), so with
--questions-per-pass 3 the passes are [1, 2, 3], [4, 6, 7], [8] (the epoch of 8 questions ends inside a window) and
[9, 10, 11] (train_reader.pass_schedule).  The runs stop after three updates (batch step 11, in the second epoch).

Within the first window no weight has changed, so the run of one question per pass and the run of three compute its three
losses on identical weights and inputs.  Each is within FORWARD_BOUNDS["loss"] of tests/test_trainable_reader_gpu.py
(relative, against float64) of the float64 loss, so the two agree within twice that bound.  Later losses are computed on
weights that went through an optimizer step of gradients that differ in their last bits: they are counted, not compared.
"""
import json
import os

import pytest

from test_train_reader_gpu import _argv, setup      # noqa: F401  (the module-scoped fixture, built again here)
from test_trainable_reader_gpu import FORWARD_BOUNDS

pytestmark = pytest.mark.gpu

FLAGS = ("--deterministic", "--learning_rate", "1e-3", "--gradient_accumulation_steps", "4", "--digest-every", "1",
         "--save-state", "--save_checkpoints_steps", "1")
G = 4


def _run(setup, out, *flags, init=True):        # noqa: F811
    from proqa_amd import train_reader
    argv = _argv(setup, out, *FLAGS, *flags)
    if not init:
        at = argv.index("--init_checkpoint")
        del argv[at:at + 2]
    stats_file = setup["root"] / f"stats-{out}.json"
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("PROQA_STATS_JSON", str(stats_file))
        train_reader.main(argv)
    finally:
        mp.undo()
    return json.loads(stats_file.read_text())


@pytest.fixture(scope="module")
def runs(gpu_device, setup):        # noqa: F811
    one = _run(setup, "multi-q1", "--stop-after-updates", "3")
    three = _run(setup, "multi-q3", "--questions-per-pass", "3", "--stop-after-updates", "3")
    return one, three


def test_three_questions_per_pass_take_the_steps_of_one(gpu_device, setup, runs):        # noqa: F811
    from proqa_amd.train_reader import pass_schedule, update_schedule
    one, three = runs
    assert one["questions_per_pass"] == 1 and three["questions_per_pass"] == 3
    for key in ("update_steps", "failed_steps", "batch_steps", "global_step", "failed_retrieval"):
        assert one[key] == three[key], key
    assert one["global_step"] == 3 and one["batch_steps"] == 11 and one["update_steps"] == update_schedule(11, G, one["failed_steps"])
    # the failed retrieval planted inside a window: the 5th question, no update slot
    assert one["failed_steps"] == [5]
    assert len(one["losses"]) == len(three["losses"]) == 11 - len(one["failed_steps"])
    first_epoch = pass_schedule(8, G, 3, failed=one["failed_steps"])
    second = pass_schedule(3, G, 3, failed=one["failed_steps"], first=9)
    assert first_epoch == [[1, 2, 3], [4, 6, 7], [8]] and second == [[9, 10, 11]]
    assert three["passes"] == len(first_epoch) + len(second) < one["passes"]
    assert one["passes"] == len(one["losses"])
    # the first window: identical weights on both sides
    bound = 2.0 * FORWARD_BOUNDS["loss"] / (1.0 - FORWARD_BOUNDS["loss"])
    for i in range(3):
        a, b = one["losses"][i], three["losses"][i]
        err = abs(a - b) / max(abs(a), abs(b))
        print(f"question {i + 1}: one per pass {a:.7f}, three per pass {b:.7f}, difference {err:.3e} allowed {bound:.3e}")
        assert err <= bound, (i, a, b)
    assert all(x == x and abs(x) < float("inf") for x in three["losses"])
    assert len({d["params"] for d in three["state_digests"]}) == 3          # the weights moved at every update
    log = open(os.path.join(three["output_dir"], "log.txt")).read()
    assert "--questions-per-pass 3" in log and "every pass holds one question" not in log


def test_resume_of_a_three_question_run(gpu_device, setup, runs):        # noqa: F811
    _, straight = runs
    half = _run(setup, "multi-q3-halves", "--questions-per-pass", "3", "--stop-after-updates", "1")
    assert half["global_step"] == 1 and half["batch_steps"] == 3 and half["stopped_early"] is True
    assert half["state_digests"] == straight["state_digests"][:1]
    resumed = _run(setup, "multi-q3-halves", "--questions-per-pass", "3", "--stop-after-updates", "3", "--resume",
                   half["output_dir"], init=False)
    for key in ("global_step", "batch_steps", "update_steps", "failed_steps", "losses", "state_digests", "loss_scale", "passes"):
        assert resumed[key] == straight[key], key
    # another --questions-per-pass is another run
    with pytest.raises(SystemExit, match="'questions_per_pass' is 1 now, was 3"):
        _run(setup, "multi-q3-halves", "--stop-after-updates", "3", "--resume", half["output_dir"], init=False)
    with pytest.raises(SystemExit, match="'questions_per_pass' is 2 now, was 3"):
        _run(setup, "multi-q3-halves", "--questions-per-pass", "2", "--stop-after-updates", "3", "--resume", half["output_dir"],
             init=False)


def test_one_question_windows_say_so_once(gpu_device, setup):        # noqa: F811
    stats = _run(setup, "multi-g1", "--questions-per-pass", "3", "--gradient_accumulation_steps", "1", "--stop-after-updates", "2")
    assert stats["passes"] == len(stats["losses"]) == 2 and stats["questions_per_pass"] == 3
    log = open(os.path.join(stats["output_dir"], "log.txt")).read()
    assert log.count("every pass holds one question") == 1
