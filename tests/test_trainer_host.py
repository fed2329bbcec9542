"""proqa_amd/trainer.py without a GPU: the early-stopping rule and its end-of-epoch variant, the save/stop rule, the refusals
both training commands share (and each command's own behind them), the merged "field defaults to 1" check of a resumed
reader run, the run directory with its log handlers, and the figures finish() leaves."""
import argparse
import itertools
import json
import logging

import pytest

from proqa_amd import config, pretrain_retriever, train_reader, trainer
from test_train_reader_host import _args as reader_args

PRETRAIN_BASE = ["--train_file", "t.txt", "--predict_file", "d.txt"]          # as tests/test_checkpoint_host.py builds them


def _run(tmp_path=None, logger=None, **flags):
    args = argparse.Namespace(**dict(dict(output_dir=str(tmp_path), wait_step=2, save_state=False, save_checkpoints_steps=1000,
                                          stop_after_updates=0, digest_every=0, resume="", deterministic=False), **flags))
    return trainer.TrainerRun("some_command.py", args, logger or logging.getLogger("test_trainer_host.unused"))


# ---- the score rule ------------------------------------------------------------------------------------------------------

SCORES = [0.5, 0.4, 0.6, 0.6, 0.6]


def test_score_rule_step_by_step():
    run = _run(wait_step=2)
    seen = []
    for s in SCORES:
        improved = run.note_score(s)
        seen.append((improved, run.best, run.wait_step, run.stop_training))
    assert seen == [(True, 0.5, 0, False), (False, 0.5, 1, False), (True, 0.6, 0, False),
                    (False, 0.6, 1, False),            # an equal score is not an improvement
                    (False, 0.6, 2, True)]
    assert run.note_score(0.6) is False and (run.wait_step, run.stop_training) == (3, True)     # == : counted on, not re-armed
    assert run.note_score(0.7) is True and (run.best, run.wait_step, run.stop_training) == (0.7, 0, False)   # cleared


def test_patience_zero_never_stops():
    run = _run(wait_step=0)
    for s in SCORES + [0.1] * 5:
        run.note_score(s)
    assert run.wait_step == 7 and run.stop_training is False


def test_end_of_epoch_variant_neither_counts_nor_clears():
    run = _run(wait_step=2)
    seen = []
    for s in SCORES:
        improved = run.note_score(s, patience=False)
        seen.append((improved, run.best, run.wait_step, run.stop_training))
    assert seen == [(True, 0.5, 0, False), (False, 0.5, 0, False), (True, 0.6, 0, False), (False, 0.6, 0, False),
                    (False, 0.6, 0, False)]
    run.wait_step, run.stop_training = 2, True
    assert run.note_score(0.5, patience=False) is False and (run.wait_step, run.stop_training) == (2, True)
    assert run.note_score(0.9, patience=False) is True
    assert (run.best, run.wait_step, run.stop_training) == (0.9, 0, True)          # the count restarts, the stop stays


# ---- the save/stop rule --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("save_state", [False, True])
def test_save_and_stop_rule(save_state):
    for global_step, every, stop_after, also in itertools.product(range(1, 9), (1, 2, 3, 1000), (0, 3, 4), (False, True)):
        run = _run(save_state=save_state, save_checkpoints_steps=every, stop_after_updates=stop_after)
        run.global_step = global_step
        want_stop = save_state and global_step == stop_after
        want_save = save_state and (global_step % every == 0 or also or want_stop)
        assert (bool(run.save_due(also=also)), run.stopped_early) == (want_save, want_stop)


# ---- the refusals ---------------------------------------------------------------------------------------------------------

SHARED_REFUSALS = [
    (["--accumulate_gradients", "0"], ValueError, "Invalid accumulate_gradients parameter: 0, should be >= 1"),
    (["--do_predict"], SystemExit, "{command}: --do_predict alone is {alone} --do_predict --init_checkpoint ..."),
    (["--train_file", ""], ValueError, "`train_file` must be specified"),
    (["--predict_file", ""], ValueError, "`predict_file` must be specified"),
    (["--local_rank", "0"], SystemExit, "{command}: --local_rank (DistributedDataParallel) is not supported: one GPU per run"),
    (["--no_cuda"], SystemExit, "{command}: --no_cuda: proqa_amd has no CPU path"),
    (["--gradient_accumulation_steps", "0"], ValueError, "Invalid gradient_accumulation_steps parameter: 0, should be >= 1"),
]
COMMANDS = {
    "pretrain_retriever.py": (lambda *argv: config.get_args(PRETRAIN_BASE + list(argv)), pretrain_retriever.check_args,
                              "the dev evaluation of a checkpoint: run train_retriever.py"),
    "train_reader.py": (reader_args, train_reader.check_args, "the evaluation of a checkpoint: run train_retrieve_qa.py"),
}


@pytest.mark.parametrize("command", sorted(COMMANDS))
@pytest.mark.parametrize("argv,error,text", SHARED_REFUSALS)
def test_shared_refusals_name_the_command(command, argv, error, text):
    get_args, check_args, alone = COMMANDS[command]
    text = text.format(command=command, alone=alone)
    with pytest.raises(error) as e:
        trainer.check_train_args(get_args(*argv), command, alone)
    assert text in str(e.value)
    with pytest.raises(error) as e:                       # and through the command's own check_args, the same text
        check_args(get_args(*argv))
    assert text in str(e.value)


def test_check_train_args_implies_do_train():
    for command, (get_args, _, alone) in COMMANDS.items():
        assert get_args().do_train is False
        assert trainer.check_train_args(get_args(), command, alone).do_train is True
        assert trainer.check_train_args(get_args("--do_train", "--do_predict"), command, alone).do_train is True


def test_each_command_keeps_its_own_refusals():
    get_args = COMMANDS["pretrain_retriever.py"][0]
    with pytest.raises(SystemExit, match="pretrain_retriever.py: a ';' list"):
        pretrain_retriever.check_args(get_args("--init_checkpoint", "a.pt;b.pt"))
    with pytest.raises(ValueError, match="leaves no example per batch"):
        pretrain_retriever.check_args(get_args("--train_batch_size", "2", "--accumulate_gradients", "4"))
    with pytest.raises(SystemExit, match="pretrain_retriever.py: --resume together with --init_checkpoint"):
        pretrain_retriever.check_args(get_args("--resume", "x.pt", "--init_checkpoint", "y.pt"))
    for argv, error, match in [(["--use-spanbert"], SystemExit, "train_reader.py: --use-spanbert"),
                               (["--separate"], SystemExit, "--separate / --add-select are not built"),
                               (["--add-select"], SystemExit, "--separate / --add-select are not built"),
                               (["--questions-per-pass", "0"], ValueError, "Invalid questions_per_pass parameter: 0"),
                               (["--sampler-lookahead", "0"], ValueError, "Invalid sampler_lookahead parameter: 0"),
                               (["--train_batch_size", "65"], ValueError, "passages per question"),
                               (["--matched-para-path", ""], ValueError, "--matched-para-path is required"),
                               (["--stop-after-updates", "-1"], SystemExit, "train_reader.py: --stop-after-updates must not")]:
        with pytest.raises(error, match=match):
            train_reader.check_args(reader_args(*argv))
    assert train_reader.check_args(reader_args("--stop-after-updates", "3")).save_state is True      # check_state_flags ran


@pytest.mark.parametrize("field", ["questions_per_pass", "sampler_lookahead"])
def test_field_that_defaults_to_one(field):
    check = train_reader.check_field_default_1
    check({}, field, 1)                                   # a state file from before the flag: written at 1
    with pytest.raises(SystemExit) as e:
        check({"seed": 3}, field, 4)
    assert str(e.value) == (f"--resume: the state file was written by a different run: field '{field}' is 4 now, was 1 "
                            "when the state was saved")
    check({field: 4}, field, 4)
    check({field: 1}, field, 1)
    with pytest.raises(SystemExit) as e:
        check({field: 4}, field, 2)
    assert str(e.value) == (f"--resume: the state file was written by a different run: field '{field}' is 2 now, was 4 "
                            "when the state was saved")


# ---- the run directory -----------------------------------------------------------------------------------------------------

def test_run_context_logs_through_the_commands_logger(tmp_path, capsys):
    logger = logging.getLogger("proqa_amd.some_command")
    out = tmp_path / "runs" / "name"
    with _run(out, logger) as run:
        assert out.is_dir() and len(logger.handlers) == 2 and logger.propagate is False
        assert {type(h) for h in logger.handlers} == {logging.FileHandler, logging.StreamHandler}
        assert logging.getLogger(trainer.__name__).handlers == []         # the module has no logger of its own to hang them on
        logger.info("first run")
        run.log_resumed("question")                                       # a line of the shared code: the same logger
    assert logger.handlers == []
    assert "already exists" not in capsys.readouterr().out
    lines = (out / "log.txt").read_text().splitlines()
    assert len(lines) == 2 and lines[0].endswith(" - INFO - proqa_amd.some_command - first run")
    assert " - INFO - proqa_amd.some_command - Resumed from " in lines[1] and ", question 0, epoch 0 position 0." in lines[1]

    closed = []
    with pytest.raises(KeyError):
        with _run(out, logger) as run:
            run.closing.append(argparse.Namespace(close=lambda: closed.append("para_db")))
            logger.info("second run")
            raise KeyError("the body fails")
    assert logger.handlers == [] and closed == ["para_db"]
    assert f"output directory {out} already exists and is not empty." in capsys.readouterr().out
    lines = (out / "log.txt").read_text().splitlines()                    # appended, not truncated
    assert len(lines) == 3 and lines[2].endswith(" - INFO - proqa_amd.some_command - second run")


# ---- finish ---------------------------------------------------------------------------------------------------------------

class _Optimizer:
    param_groups = []

    def state_dict(self):
        return {"fused": {"step": 5, "skipped_steps": 1, "clean_steps": 4, "loss_scale": 32768.0}}


@pytest.mark.parametrize("stop_after,digest_every", [(0, 0), (5, 0), (0, 2), (5, 2)])
def test_finish_fills_the_commands_dict_in_place(tmp_path, monkeypatch, stop_after, digest_every):
    monkeypatch.setenv("PROQA_STATS_JSON", str(tmp_path / "stats.json"))
    run = _run(tmp_path, stop_after_updates=stop_after, digest_every=digest_every, deterministic=True)
    if digest_every == 0:
        assert run.attach(None, _Optimizer(), 0, lambda: pytest.fail("no state flag: the order is not asked for")) is None
        assert run.ckpt is None and run.digests is None and run.state_path == str(tmp_path / "trainer_state_last.pt")
    run.optimizer = _Optimizer()           # (with --digest-every attach() builds the device-side checkpoint: not here)
    run.digests = argparse.Namespace(entries=[{"step": 2, "params": 1, "exp_avg": 2, "exp_avg_sq": 3}])
    run.global_step, run.batch_step, run.stopped_early = 5, 10, stop_after > 0
    run.meter.values, run.evals = [1.5, 0.5], [{"step": 4, "acc": 0.25}]
    stats = {"stale": True}
    assert run.finish(stats, best_acc=0.25) is stats
    keys = {"global_step", "batch_steps", "losses", "evals", "skipped_steps", "loss_scale", "seconds", "output_dir",
            "deterministic", "best_acc"}
    assert set(stats) == keys | ({"stopped_early"} if stop_after > 0 else set()) | ({"state_digests"} if digest_every > 0 else set())
    assert (stats["global_step"], stats["batch_steps"], stats["losses"], stats["skipped_steps"], stats["loss_scale"]) == \
        (5, 10, [1.5, 0.5], 1, 32768.0)
    assert stats["output_dir"] == str(tmp_path) and stats["deterministic"] is True and stats["seconds"] >= 0
    assert stats.get("stopped_early", True) is True and stats.get("state_digests", run.digests.entries) == run.digests.entries
    assert json.loads((tmp_path / "stats.json").read_text()) == stats
