"""Training with deterministic=True / --deterministic: the word-embedding gradient is summed in a fixed order, so a run is a
function of (data, seed, checkpoint) bit for bit with NO parameter frozen -- the modules (three optimizer steps of two fresh
models) and the two commands (two runs of one seed).  Dropout is on wherever the tiny configurations have it: the masks are
recomputed from (seed, call) and are part of what must reproduce.

The word tables' gradients are compared with the default (atomic) mode's under the d_word bounds of
tests/test_embed_word_grad_gpu.py (the measured fp16-storage error of the reference arithmetic x 4): both modes sum the same
fp32 terms, in different orders.  Every other gradient carries the default mode's bits.
"""
import json
import os

import pytest
import torch

import reader_train_oracle
import train_oracle
from test_embed_word_grad_gpu import D_WORD_BOUND
from test_pretrain_retriever_gpu import _run as run_pretrain
from test_pretrain_retriever_gpu import setup as pretrain_setup  # noqa: F401  (a fixture)
from test_train_reader_gpu import _run as run_train_reader
from test_train_reader_gpu import setup as reader_setup  # noqa: F401  (a fixture)
from proqa_amd.reader import random_state_dict as reader_state_dict
from proqa_amd.retriever import random_state_dict as retriever_state_dict

pytestmark = pytest.mark.gpu

CFG = train_oracle.SMALL_CONFIG
RATES = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
STEPS = 3


def bits(t):
    return t.view(torch.int32)


def on(dev, batch):
    return {k: v.to(dev) for k, v in batch.items()}


def retriever_batch():
    """small_batch: 8 pairs over a vocabulary of 120 (every word piece repeats within and across the sequences), with one
    [CLS]-like id at position 0 of every sequence"""
    batch = {k: v.clone() for k, v in train_oracle.small_batch(0).items()}
    batch["input_ids_q"][:, 0] = 1
    batch["input_ids_c"][:, 0] = 1
    return batch


def retriever_model(dev, deterministic):
    from proqa_amd.trainable import TrainableRetriever
    model = TrainableRetriever(CFG, device=dev, dropout_seed=11, deterministic=deterministic, **RATES)
    model.load_state_dict(retriever_state_dict(CFG, seed=0))
    return model.train()


def retriever_loss(model, batch):
    from proqa_amd.trainable import inbatch_loss
    out = model(batch)
    return inbatch_loss(out["q"], out["c"])


def reader_model(dev, deterministic):
    from proqa_amd.trainable_reader import TrainableReader
    model = TrainableReader(CFG, device=dev, dropout_seed=11, qa_drop=0.1, deterministic=deterministic, **RATES)
    model.load_state_dict(reader_state_dict(CFG, seed=0))
    return model.train()


def reader_loss(model, batch):
    return model(batch)["loss"]


def first_gradients(model, loss_of, batch):
    model.zero_grad(set_to_none=True)
    (loss_of(model, batch) * 1024.0).backward()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def train(model, loss_of, batch):
    from proqa_amd.optim import FusedAdamW
    opt = FusedAdamW([p for p in model.parameters()], lr=1e-3, max_grad_norm=2.0, loss_scale="dynamic")
    losses = []
    for _ in range(STEPS):
        loss = loss_of(model, batch)
        losses.append(loss.item())
        opt.scale_loss(loss).backward()
        opt.step()
        opt.zero_grad()
    return losses, {k: p.detach().clone() for k, p in model.named_parameters()}


def check_module(dev, make, loss_of, batch, typed_prefix):
    batch = on(dev, batch)
    # the gradients of the first step, from the same weights and masks: deterministic against default
    det, default = first_gradients(make(dev, True), loss_of, batch), first_gradients(make(dev, False), loss_of, batch)
    assert set(det) == set(default)
    tables = [k for k in det if "word_embeddings" in k]
    assert tables
    for k in det:
        if k in tables:
            bound = D_WORD_BOUND[k.startswith(typed_prefix)]
            err = train_oracle.rel_err(det[k].cpu(), default[k].cpu())
            print(f"{k}: deterministic against atomic {err:.3e} bound {bound:.3e}")
            assert err <= bound, (k, err, bound)
            assert (det[k] != 0).any()
        else:
            assert torch.equal(bits(det[k]), bits(default[k])), k
    # three steps of two fresh models: every parameter, the word tables included
    a, b = make(dev, True), make(dev, True)
    assert a.deterministic and not make(dev, False).deterministic
    losses_a, params_a = train(a, loss_of, batch)
    losses_b, params_b = train(b, loss_of, batch)
    assert losses_a == losses_b and all(x == x for x in losses_a)
    for k in params_a:
        assert torch.equal(bits(params_a[k]), bits(params_b[k])), k
    start = make(dev, True)
    for k in tables:                                  # and the tables did move
        assert not torch.equal(params_a[k], dict(start.named_parameters())[k].detach()), k


def test_retriever_module_reproduces_every_parameter(gpu_device):
    check_module(gpu_device, retriever_model, retriever_loss, retriever_batch(), typed_prefix="\0")


def test_reader_module_reproduces_every_parameter(gpu_device):
    from proqa_amd.trainable_reader import TrainableReader
    check_module(gpu_device, reader_model, reader_loss, reader_train_oracle.SMALL_READER_BATCH, typed_prefix="bert.")
    model = TrainableReader(CFG, device=gpu_device, deterministic=True)
    assert model.deterministic and model.retriever.deterministic
    args = type("Args", (), {"deterministic": True, "shared_norm": True})()
    assert TrainableReader.from_args(CFG, args, gpu_device).deterministic
    assert not TrainableReader.from_args(CFG, type("Args", (), {})(), gpu_device).deterministic


def _same_checkpoint(path_a, path_b):
    a, b = torch.load(path_a, map_location="cpu"), torch.load(path_b, map_location="cpu")
    assert set(a) == set(b) and any("word_embeddings" in k for k in a)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    return a


def test_pretrain_retriever_command_reproduces_a_run(gpu_device, pretrain_setup, monkeypatch):  # noqa: F811
    from proqa_amd import pretrain_retriever
    assert pretrain_retriever.FROZEN_PARAMETERS == ()
    flags = ("--learning_rate", "1e-3", "--num_train_epochs", "3", "--eval-period", "3", "--deterministic")
    a = run_pretrain(pretrain_setup, "deterministic-a", monkeypatch, *flags, model="drop")
    b = run_pretrain(pretrain_setup, "deterministic-b", monkeypatch, *flags, model="drop")
    assert a["deterministic"] is True and b["deterministic"] is True
    assert len(a["losses"]) == 12 and all(x == x and abs(x) < float("inf") for x in a["losses"])
    assert a["losses"] == b["losses"] and a["global_step"] == b["global_step"] == 6
    last = _same_checkpoint(os.path.join(a["output_dir"], "checkpoint_last.pt"), os.path.join(b["output_dir"], "checkpoint_last.pt"))
    start = pretrain_setup["sd"]
    key = "bert_q.embeddings.word_embeddings.weight"
    assert not torch.equal(last[key], start[key])                    # the tables were trained
    log = open(os.path.join(a["output_dir"], "log.txt")).read()
    assert "word-embedding gradient is summed in a fixed order" in log
    plain = run_pretrain(pretrain_setup, "deterministic-off", monkeypatch, "--learning_rate", "1e-3", "--num_train_epochs", "1",
                         model="drop")
    assert plain["deterministic"] is False
    assert "fixed order" not in open(os.path.join(plain["output_dir"], "log.txt")).read()


def test_train_reader_command_reproduces_a_run(gpu_device, reader_setup, monkeypatch):  # noqa: F811
    from proqa_amd import train_reader
    assert train_reader.FROZEN_PARAMETERS == ()
    flags = ("--learning_rate", "1e-3", "--qa-drop", "0.1", "--deterministic")
    a = run_train_reader(reader_setup, "deterministic-a", monkeypatch, *flags)
    b = run_train_reader(reader_setup, "deterministic-b", monkeypatch, *flags)
    assert a["deterministic"] is True and b["deterministic"] is True
    assert len(a["losses"]) > 4 and all(x == x and abs(x) < float("inf") for x in a["losses"])
    assert a["losses"] == b["losses"] and a["failed_steps"] == b["failed_steps"]
    assert [e["em"] for e in a["evals"]] == [e["em"] for e in b["evals"]]
    best = _same_checkpoint(os.path.join(a["output_dir"], "best-model.pt"), os.path.join(b["output_dir"], "best-model.pt"))
    start = reader_setup["sd"]
    assert not torch.equal(best["bert.embeddings.word_embeddings.weight"], start["bert.embeddings.word_embeddings.weight"])
    assert "word-embedding gradient is summed in a fixed order" in open(os.path.join(a["output_dir"], "log.txt")).read()
    assert json.loads((reader_setup["root"] / "stats-deterministic-a.json").read_text())["deterministic"] is True
