"""--stop-after-updates / --resume / --digest-every of the two training commands on the tiny models and synthetic files of
tests/test_pretrain_retriever_gpu.py and tests/test_train_reader_gpu.py.  With --deterministic a run that is stopped after
K updates and resumed ends in the state of the uninterrupted run, bit for bit: the final state files hold the same masters,
moments, optimizer scalars and digests, the stats the same losses and per-step state digests."""
import json
import os
import shutil

import pytest
import torch

from test_pretrain_retriever_gpu import setup as pretrain_setup      # noqa: F401  (module-scoped fixtures, built again here)
from test_pretrain_retriever_gpu import _run as run_pretrain
from test_train_reader_gpu import CFG as READER_CFG, GOLDEN, SEED as READER_SEED, _argv as reader_argv
from test_train_reader_gpu import setup as reader_setup              # noqa: F401

pytestmark = pytest.mark.gpu

K = 3            # the pre-training epoch is 4 micro-batches = 2 updates (G = 2): the third update lies inside the second epoch
PRETRAIN_FLAGS = ("--deterministic", "--learning_rate", "1e-3", "--num_train_epochs", "3", "--digest-every", "1",
                  "--eval-period", "2")
TRAINER_FIELDS = ("global_step", "batch_step", "epoch", "position", "epoch_started", "best", "wait_step", "stop_training",
                  "dropout", "losses", "loss_steps", "evals", "fused", "state_digests", "param_groups", "reader", "fingerprint")


def _state(run_dir):
    from proqa_amd import checkpoint
    return checkpoint.read_state(checkpoint.resolve_state_path(run_dir))


def _assert_same_state(a, b):
    """masters, both moments, the optimizer's scalars, the digests and the counters of two state files, bit for bit"""
    assert a["names"] == b["names"] and a["offsets"] == b["offsets"] and a["shapes"] == b["shapes"]
    assert torch.equal(a["digests"], b["digests"])
    assert torch.equal(a["flat"], b["flat"])
    for k in TRAINER_FIELDS:
        assert a["trainer"][k] == b["trainer"][k], k
    assert a["trainer"]["fused"]["step"] >= 1


# ---- pretrain_retriever.py ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pretrain_runs(gpu_device, pretrain_setup):          # noqa: F811
    """the straight run of 2K updates, and the run stopped after K; both with dropout 0.1 / 0.1 and G = 2"""
    mp = pytest.MonkeyPatch()
    try:
        straight = run_pretrain(pretrain_setup, "resume-straight", mp, *PRETRAIN_FLAGS, "--stop-after-updates", str(2 * K),
                                model="drop")
        half = run_pretrain(pretrain_setup, "resume-halves", mp, *PRETRAIN_FLAGS, "--stop-after-updates", str(K), model="drop")
    finally:
        mp.undo()
    return straight, half


def test_pretrain_resumed_run_equals_the_straight_run(gpu_device, pretrain_setup, pretrain_runs, monkeypatch):      # noqa: F811
    straight, half = pretrain_runs
    assert straight["global_step"] == 2 * K and straight["stopped_early"] is True and straight["batch_steps"] == 4 * K - 1
    assert half["global_step"] == K and half["stopped_early"] is True and half["batch_steps"] == 2 * K - 1
    first = _state(half["output_dir"])["trainer"]
    assert (first["epoch"], first["position"]) == (1, 1) and first["global_step"] == K       # inside the second epoch
    resumed = run_pretrain(pretrain_setup, "resume-halves", monkeypatch, *PRETRAIN_FLAGS, "--stop-after-updates", str(2 * K),
                           "--resume", half["output_dir"], model="drop", init=False)
    assert resumed["output_dir"] == half["output_dir"] and resumed["global_step"] == 2 * K
    assert resumed["batch_steps"] == straight["batch_steps"]
    assert resumed["losses"] == straight["losses"] and len(straight["losses"]) == 4 * K - 1
    assert resumed["losses"][:len(half["losses"])] == half["losses"]
    assert [d["step"] for d in straight["state_digests"]] == list(range(1, 2 * K + 1))
    assert resumed["state_digests"] == straight["state_digests"]
    assert half["state_digests"] == straight["state_digests"][:K]
    assert len({d["params"] for d in straight["state_digests"]}) == 2 * K             # the weights moved at every update
    assert resumed["evals"] == straight["evals"] and [e["step"] for e in straight["evals"]] == [2, 4, 6]
    assert resumed["best_acc"] == straight["best_acc"] and resumed["loss_scale"] == straight["loss_scale"]
    _assert_same_state(_state(straight["output_dir"]), _state(resumed["output_dir"]))
    log = open(os.path.join(half["output_dir"], "log.txt")).read()           # appended to, not replaced
    assert log.count("Start training....") == 2 and "Resumed from" in log and "bit for bit as the uninterrupted one" in log
    assert log.count("state digest at step") == 2 * K
    # the model files of the reference are still written, and a state file is no model checkpoint
    assert os.path.isfile(os.path.join(half["output_dir"], "checkpoint_last.pt"))


def test_pretrain_state_file_contents(gpu_device, pretrain_runs):
    import numpy as np
    import state_digest_oracle as oracle
    from proqa_amd import checkpoint
    from proqa_amd.trainable import state_dict_keys
    from test_pretrain_retriever_gpu import CFG
    straight, _ = pretrain_runs
    obj = _state(straight["output_dir"])
    keys = state_dict_keys(CFG)
    assert obj["names"] == ["model." + k for k in keys] + ["exp_avg." + k for k in _by_group(keys)] + \
        ["exp_avg_sq." + k for k in _by_group(keys)] + [checkpoint.DEVICE_STATE]
    tensors = checkpoint.state_tensors(obj)
    last = torch.load(os.path.join(straight["output_dir"], "checkpoint_last.pt"), map_location="cpu")
    for k in keys:          # checkpoint_last.pt was written at the same update
        assert torch.equal(tensors["model." + k], last[k]), k
    for name, d in zip(obj["names"], obj["digests"].tolist()):          # the file's digests are the oracle's of its bytes
        assert d & ((1 << 64) - 1) == oracle.digest(tensors[name].contiguous().numpy().view(np.uint32)), name
    assert obj["trainer"]["fused"] == {"step": 2 * K, "skipped_steps": 0, "clean_steps": 2 * K, "loss_scale": 65536.0}
    assert obj["trainer"]["state_digests"][-1]["params"] == checkpoint.combine_digests(
        obj["digests"][:len(keys)].tolist())
    assert all(o % 256 == 0 for o in obj["offsets"])


def _by_group(keys):
    """the optimizer's order: the decayed group, then biases and LayerNorm weights"""
    no_decay = ("bias", "LayerNorm.weight")
    return [k for k in keys if not any(nd in k for nd in no_decay)] + [k for k in keys if any(nd in k for nd in no_decay)]


def test_pretrain_refusals(gpu_device, pretrain_setup, pretrain_runs, monkeypatch):       # noqa: F811
    from proqa_amd import checkpoint
    _, half = pretrain_runs
    flags = PRETRAIN_FLAGS + ("--stop-after-updates", str(2 * K))
    with pytest.raises(SystemExit, match="'seed' is 12 now, was 11"):
        run_pretrain(pretrain_setup, "refused", monkeypatch, *flags, "--resume", half["output_dir"], "--seed", "12",
                     model="drop", init=False)
    with pytest.raises(SystemExit, match="'train_batch_size' is 8 now, was 16"):
        run_pretrain(pretrain_setup, "refused", monkeypatch, *flags, "--resume", half["output_dir"], "--train_batch_size", "8",
                     model="drop", init=False)
    with pytest.raises(SystemExit, match="'hidden_dropout_prob'"):
        run_pretrain(pretrain_setup, "refused", monkeypatch, *flags, "--resume", half["output_dir"], model="nodrop", init=False)
    with pytest.raises(SystemExit, match="--resume together with --init_checkpoint"):
        run_pretrain(pretrain_setup, "refused", monkeypatch, *flags, "--resume", half["output_dir"], model="drop")
    with pytest.raises(SystemExit, match="already holds"):
        run_pretrain(pretrain_setup, "refused", monkeypatch, *PRETRAIN_FLAGS, "--stop-after-updates", str(K), "--resume",
                     half["output_dir"], model="drop", init=False)
    # one flipped byte inside a tensor: the digest check names the tensor
    obj = _state(half["output_dir"])
    victim = 5
    obj["flat"] = obj["flat"].clone()
    obj["flat"][obj["offsets"][victim] + 1] ^= 0x10
    damaged = str(pretrain_setup["root"] / "damaged_state.pt")
    checkpoint.atomic_save(obj, damaged)
    with pytest.raises(SystemExit, match=f"tensor '{obj['names'][victim]}' does not have the digest"):
        run_pretrain(pretrain_setup, "refused", monkeypatch, *flags, "--resume", damaged, model="drop", init=False)


# ---- train_reader.py ---------------------------------------------------------------------------------------------------------

READER_FLAGS = ("--deterministic", "--learning_rate", "1e-3", "--gradient_accumulation_steps", "2", "--digest-every", "1",
                "--save-state", "--save_checkpoints_steps", "1")


def _run_reader(setup, model_dir, out, *flags, init=True):
    from proqa_amd import train_reader
    argv = reader_argv(setup, out, *flags)
    argv[argv.index("--bert_model_name") + 1] = model_dir
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
def reader_runs(gpu_device, reader_setup):            # noqa: F811
    """-> (model directory with both dropout rates 0.1, the straight run over two epochs, the number of updates after
    which the interrupted run stops: the first update of the second epoch that is not that epoch's first question)"""
    d = reader_setup["root"] / "small-bert-drop"
    d.mkdir()
    shutil.copy(os.path.join(GOLDEN, "vocab_small.txt"), d / "vocab.txt")
    (d / "config.json").write_text(json.dumps(dict(READER_CFG, model_type="bert", hidden_dropout_prob=0.1,
                                                   attention_probs_dropout_prob=0.1)))
    straight = _run_reader(reader_setup, str(d), "resume-straight", *READER_FLAGS)
    inside = [i + 1 for i, b in enumerate(straight["update_steps"]) if 10 <= b <= 15]
    assert inside, straight["update_steps"]
    return str(d), straight, inside[0]


def test_reader_resumed_run_equals_the_straight_run(gpu_device, reader_setup, reader_runs):        # noqa: F811
    model_dir, straight, k = reader_runs
    assert straight["batch_steps"] == 16 and straight["global_step"] == len(straight["update_steps"]) > k
    half = _run_reader(reader_setup, model_dir, "resume-halves", *READER_FLAGS, "--stop-after-updates", str(k))
    assert half["stopped_early"] is True and half["global_step"] == k
    assert half["update_steps"] == straight["update_steps"][:k] and 9 < half["batch_steps"] < 16      # in the second epoch
    # a failed retrieval lies before the resume point (the question without an answer anywhere, in the first epoch)
    assert half["failed_steps"] and half["failed_steps"][0] < half["update_steps"][-1]
    first = _state(half["output_dir"])["trainer"]
    assert first["epoch"] == 1 and first["position"] == half["batch_steps"] - 8 and first["epoch_started"] is True
    assert sorted(first["reader"]["permutation"]) == list(range(8)) and first["reader"]["permutation"] != list(range(8))
    resumed = _run_reader(reader_setup, model_dir, "resume-halves", *READER_FLAGS, "--resume",
                          os.path.join(half["output_dir"], "trainer_state_last.pt"), init=False)
    assert resumed["output_dir"] == half["output_dir"]
    for key in ("global_step", "batch_steps", "update_steps", "failed_steps", "failed_retrieval", "losses", "state_digests",
                "loss_scale", "skipped_steps", "best_em"):
        assert resumed[key] == straight[key], key
    assert [e["em"] for e in resumed["evals"]] == [e["em"] for e in straight["evals"]] and len(straight["evals"]) == 2
    assert [d["step"] for d in straight["state_digests"]] == list(range(1, straight["global_step"] + 1))
    # the weights moved at every update but those the dynamic loss scale skipped (an overflow leaves p, m and v as they are)
    assert len({d["params"] for d in straight["state_digests"]}) == straight["global_step"] - straight["skipped_steps"]
    assert "stopped_early" not in resumed
    _assert_same_state(_state(straight["output_dir"]), _state(resumed["output_dir"]))
    log = open(os.path.join(half["output_dir"], "log.txt")).read()
    assert log.count("Start training....") == 2 and "Resumed from" in log and log.count("Failed retrieval:") == 2


def test_reader_refuses_another_seed(gpu_device, reader_setup, reader_runs):          # noqa: F811
    model_dir, straight, _ = reader_runs
    with pytest.raises(SystemExit, match=f"'seed' is 5 now, was {READER_SEED}"):
        _run_reader(reader_setup, model_dir, "refused", *READER_FLAGS, "--resume", straight["output_dir"], "--seed", "5",
                    init=False)
    with pytest.raises(SystemExit, match="'gradient_accumulation_steps'"):
        _run_reader(reader_setup, model_dir, "refused", *READER_FLAGS, "--resume", straight["output_dir"],
                    "--gradient_accumulation_steps", "1", init=False)
