"""Several micro-batches per tower pass: TrainableRetriever.forward on a list of batches with inbatch_loss_blocks, and
pretrain_retriever.py --micro-batches-per-pass on the tiny model and files of tests/test_pretrain_retriever_gpu.py.

The module.  A fused pass over [b0, b1, b2] is ONE pass, so it is held to what a single pass is held to in
tests/test_trainable_gpu.py and to nothing wider: the q / c rows against the sequential passes within TOL_GOLDEN, the
per-block losses within 1e-3, and the accumulated parameter gradients of BOTH routes against the float64 tower oracle
(the sum of its per-batch gradients over G) with that file's BOUNDS per kind of parameter, at its loss scale.

The command.  M = 1 is a run without the flag bit for bit (--deterministic); M = 4 forms the passes of pass_schedule,
resumes to the digests of the uninterrupted run and refuses another M; its first window reads the weights the M = 1 run
reads, so those per-micro-batch losses agree within 1e-3.
"""
import functools
import os

import pytest
import torch

import train_oracle as oracle
from test_pretrain_retriever_gpu import _run as run_pretrain
from test_pretrain_retriever_gpu import setup as pretrain_setup      # noqa: F401  (module-scoped fixture, built again here)
from test_trainable_gpu import BOUNDS, CFG, L, LOSS_SCALE, NH, kind, make_model, on
from proqa_amd.retriever import random_state_dict

pytestmark = pytest.mark.gpu

G = 4             # the accumulation window the three batches belong to
PAIRS = (8, 5, 11)


@functools.lru_cache(maxsize=None)
def reference():
    """(state dict, [three CPU batches], float64 per-batch losses, float64 accumulated gradients of sum_m loss_m / G)"""
    sd = random_state_dict(CFG, seed=0)
    batches = [oracle.small_batch(seed, pairs) for seed, pairs in enumerate(PAIRS)]
    # the second batch narrower than the others: forward right-pads it on the device
    wq, wc = int(batches[1]["input_mask_q"].sum(1).max()), int(batches[1]["input_mask_c"].sum(1).max())
    batches[1] = {k: v[:, :(wq if k.endswith("_q") else wc)].contiguous() for k, v in batches[1].items()}
    losses, total = [], None
    for b in batches:
        loss, grads, _ = oracle.model_gradients(sd, b, L, NH)
        losses.append(loss)
        total = grads if total is None else {k: total[k] + grads[k] for k in grads}
    return sd, batches, losses, {k: v / G for k, v in total.items()}


def check_gradients(model, ref, label):
    grads = {k: p.grad.detach().cpu().double() / LOSS_SCALE for k, p in model.named_parameters()}
    failures = []
    for k, want in ref.items():
        if k.endswith("attention.self.key.bias"):          # exactly zero in the oracle: relative to its layer's other biases
            layer = k[:-len("key.bias")]
            scale = max(ref[layer + "query.bias"].abs().max().item(), ref[layer + "value.bias"].abs().max().item())
            err = grads[k].abs().max().item() / scale
            bound = max(BOUNDS[kind(layer + "query.bias")], BOUNDS[kind(layer + "value.bias")])
        elif k == "proj_c.bias":                            # zero as well: relative to proj_q.bias
            err, bound = grads[k].abs().max().item() / ref["proj_q.bias"].abs().max().item(), BOUNDS["proj.bias"]
        else:
            err, bound = oracle.rel_err(grads[k], want), BOUNDS[kind(k)]
        print(f"{label} {k}: error {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            failures.append((label, k, err, bound))
    assert not failures, failures


def test_a_list_of_batches_is_one_pass_per_tower(gpu_device):
    from test_encoder_gpu import TOL_GOLDEN
    from proqa_amd.trainable import inbatch_loss, inbatch_loss_blocks
    sd, batches, want_losses, ref = reference()
    dev_batches = [on(gpu_device, b) for b in batches]

    fused = make_model(gpu_device, sd)
    out = fused(dev_batches)
    assert set(out) == {"q", "c", "block_sizes"} and out["block_sizes"] == list(PAIRS)
    assert out["q"].shape == out["c"].shape == (sum(PAIRS), 128) and out["q"].dtype == torch.float16
    losses = inbatch_loss_blocks(out["q"], out["c"], out["block_sizes"])
    ((losses / G).sum() * LOSS_SCALE).backward()

    sequential = make_model(gpu_device, sd)
    rows, seq_losses = {"q": [], "c": []}, []
    for b in dev_batches:
        o = sequential(b)
        loss = inbatch_loss(o["q"], o["c"])
        (loss / G * LOSS_SCALE).backward()
        seq_losses.append(float(loss.detach()))
        for k in rows:
            rows[k].append(o[k].detach())
    for k in rows:
        err = float((out[k].detach().float() - torch.cat(rows[k]).float()).abs().max())
        print(k, "fused against sequential rows: max abs difference", err, "bound", TOL_GOLDEN)
        assert err < TOL_GOLDEN
    for m, (a, b, want) in enumerate(zip(losses.tolist(), seq_losses, want_losses)):
        print(f"block {m}: fused loss {a:.6f} sequential {b:.6f} float64 {want:.6f}")
        assert abs(a - b) <= 1e-3 and abs(a - want) <= 2e-3          # (2e-3: the oracle figure of tests/test_trainable_gpu.py)
    check_gradients(fused, ref, "fused")
    check_gradients(sequential, ref, "sequential")
    # a single dict keeps today's path
    assert set(fused(dev_batches[0])) == {"q", "c"}
    with pytest.raises(ValueError, match="empty list"):
        fused([])


def test_dropout_takes_one_call_per_tower_pass(gpu_device):
    from proqa_amd.trainable import TrainableRetriever
    sd, batches, *_ = reference()
    model = TrainableRetriever(CFG, device=gpu_device, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                               dropout_seed=5)
    model.load_state_dict(sd)
    model.train()
    dev_batches = [on(gpu_device, b) for b in batches]
    seed, call = model.dropout_state()
    out = model(dev_batches)
    assert model.dropout_state() == (seed, call + 2)                  # one per tower pass, not one per micro-batch
    assert bool(torch.isfinite(out["q"]).all()) and bool(torch.isfinite(out["c"]).all())
    for b in dev_batches:
        model(b)
    assert model.dropout_state() == (seed, call + 2 + 2 * len(batches))
    model.set_dropout_state((seed, call))                               # the same coordinates: the same masks, the same bits
    again = model(dev_batches)
    assert torch.equal(again["q"].view(torch.int16), out["q"].view(torch.int16))


# ---- the command ---------------------------------------------------------------------------------------------------------------

FLAGS = ("--deterministic", "--learning_rate", "1e-3", "--num_train_epochs", "3", "--digest-every", "1", "--eval-period", "2",
         "--gradient_accumulation_steps", "4")
N_BATCHES = 4           # 32 pairs in micro-batches of 16 / 2


def _loss_lines(stats):
    with open(os.path.join(stats["output_dir"], "log.txt")) as f:
        return [line.split(" - ", 3)[-1] for line in f if "Train loss" in line]


def _schedule(epochs, G_, M):
    from proqa_amd.pretrain_retriever import pass_schedule
    return [p for e in range(epochs) for p in pass_schedule(N_BATCHES, G_, M, first=1 + e * N_BATCHES)]


@pytest.fixture(scope="module")
def runs(gpu_device, pretrain_setup):          # noqa: F811
    """without the flag, M = 1 and M = 4, all at G = 4 over three epochs without dropout"""
    mp = pytest.MonkeyPatch()
    try:
        plain = run_pretrain(pretrain_setup, "passes-plain", mp, *FLAGS)
        one = run_pretrain(pretrain_setup, "passes-m1", mp, *FLAGS, "--micro-batches-per-pass", "1")
        four = run_pretrain(pretrain_setup, "passes-m4", mp, *FLAGS, "--micro-batches-per-pass", "4")
    finally:
        mp.undo()
    return plain, one, four


def test_m_1_is_the_run_without_the_flag(gpu_device, runs):
    plain, one, _ = runs
    assert plain["state_digests"] == one["state_digests"] and len(plain["state_digests"]) == 3
    assert _loss_lines(plain) == _loss_lines(one) and len(_loss_lines(plain)) == 1            # (the evaluation at update 2)
    timing = ("seconds", "output_dir")
    assert {k: v for k, v in plain.items() if k not in timing} == {k: v for k, v in one.items() if k not in timing}
    assert "micro_batches_per_pass" not in one and "passes" not in one


def test_m_4_forms_the_passes_of_the_schedule(gpu_device, runs):
    from proqa_amd.pretrain_retriever import update_schedule
    plain, _, four = runs
    assert four["micro_batches_per_pass"] == 4 and four["passes"] == _schedule(3, 4, 4)
    assert four["passes"] == [[1, 2, 3], [4], [5, 6, 7], [8], [9, 10, 11], [12]]
    updates = update_schedule(3 * N_BATCHES, 4)
    assert four["global_step"] == len(updates) == 3 == plain["global_step"]
    assert set(updates) <= {p[-1] for p in four["passes"]}
    assert [d["step"] for d in four["state_digests"]] == [1, 2, 3]
    assert four["batch_steps"] == 12 == len(four["losses"])                  # one loss per micro-batch
    assert all(x == x and abs(x) < float("inf") for x in four["losses"])
    assert four["peak_memory_bytes"] > 0
    log = open(os.path.join(four["output_dir"], "log.txt")).read()
    assert log.count("share one pass per tower") == 1 and log.count("peak device allocation") == 1
    # the first window reads the weights the M = 1 run reads
    worst = max(abs(a - b) for a, b in zip(four["losses"][:3], plain["losses"][:3]))
    print("first window", four["losses"][:3], plain["losses"][:3], "largest difference", worst)
    assert worst <= 1e-3


def test_g_1_gives_singleton_passes(gpu_device, pretrain_setup, monkeypatch):          # noqa: F811
    flags = ("--deterministic", "--learning_rate", "1e-3", "--num_train_epochs", "1", "--digest-every", "1",
             "--gradient_accumulation_steps", "1")
    plain = run_pretrain(pretrain_setup, "passes-g1-plain", monkeypatch, *flags)
    four = run_pretrain(pretrain_setup, "passes-g1-m4", monkeypatch, *flags, "--micro-batches-per-pass", "4")
    assert four["passes"] == [[1], [2], [3], [4]] and four["global_step"] == 4
    assert four["state_digests"] == plain["state_digests"] and four["losses"] == plain["losses"]
    assert open(os.path.join(four["output_dir"], "log.txt")).read().count("every pass holds one micro-batch") == 1


def test_a_resumed_run_forms_the_same_passes(gpu_device, pretrain_setup, monkeypatch):          # noqa: F811
    flags = FLAGS + ("--micro-batches-per-pass", "4")
    straight = run_pretrain(pretrain_setup, "passes-straight", monkeypatch, *flags, "--stop-after-updates", "3", model="drop")
    half = run_pretrain(pretrain_setup, "passes-halves", monkeypatch, *flags, "--stop-after-updates", "2", model="drop")
    assert half["global_step"] == 2 and half["passes"] == [[1, 2, 3], [4], [5, 6, 7]]
    with pytest.raises(SystemExit, match="micro_batches_per_pass"):
        run_pretrain(pretrain_setup, "passes-refused", monkeypatch, *FLAGS, "--micro-batches-per-pass", "2",
                     "--stop-after-updates", "3", "--resume", half["output_dir"], model="drop", init=False)
    with pytest.raises(SystemExit, match="micro_batches_per_pass"):
        run_pretrain(pretrain_setup, "passes-refused", monkeypatch, *FLAGS, "--stop-after-updates", "3", "--resume",
                     half["output_dir"], model="drop", init=False)
    resumed = run_pretrain(pretrain_setup, "passes-halves", monkeypatch, *flags, "--stop-after-updates", "3", "--resume",
                           half["output_dir"], model="drop", init=False)
    assert resumed["passes"] == [[8], [9, 10, 11]]
    assert half["passes"] + resumed["passes"] == straight["passes"]
    assert resumed["state_digests"] == straight["state_digests"] and len(straight["state_digests"]) == 3
    assert resumed["losses"] == straight["losses"] and len(straight["losses"]) == 11
