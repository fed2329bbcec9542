"""TrainableRetriever.half_weights() + FusedAdamW(half_copies=...): fp16 working copies of the weight matrices, written by
the optimizer step, against the per-forward casts of the same module (train_oracle.SMALL_CONFIG, 8 pairs).

Nothing here has a tolerance.  The copy of a master is the master rounded to fp16 by the same rule as the per-forward
cast, the products take the same operands, and every other operator is untouched: losses and masters must agree bit for
bit.  The word-embedding tables are frozen in the training comparison: their gradient is summed with atomics, the
module's one run-to-run difference.
"""
import pytest
import torch

import train_oracle as oracle
from proqa_amd.retriever import random_state_dict

pytestmark = pytest.mark.gpu

CFG = oracle.SMALL_CONFIG


def _on(dev, batch):
    return {k: v.to(dev) for k, v in batch.items()}


def _model(dev, sd, freeze_words=False):
    from proqa_amd.trainable import TrainableRetriever
    model = TrainableRetriever(CFG, device=dev)
    model.load_state_dict(sd)
    if freeze_words:
        for name, p in model.named_parameters():
            if "word_embeddings" in name:
                p.requires_grad_(False)
    return model


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _forward_bits(model, batch):
    with torch.no_grad():
        out = model(batch)
    return torch.cat([_bits(out["q"]), _bits(out["c"])])


def test_layout_of_the_copies(gpu_device):
    sd = random_state_dict(CFG, seed=0)
    model = _model(gpu_device, sd)
    copies = model.half_weights()
    names = {id(p): n for n, p in model.named_parameters()}
    got = sorted(names[id(p)] for p in copies)
    want = sorted(k for k in sd if k.endswith(".weight") and "LayerNorm" not in k and "embeddings" not in k)
    assert got == want and len(got) == 2 * (6 * CFG["num_hidden_layers"] + 2)
    flat = model._half.flat
    lo, hi = flat.data_ptr(), flat.data_ptr() + 2 * flat.numel()
    for p, h in copies.items():
        assert h.dtype == torch.float16 and h.shape == p.shape and h.is_contiguous() and h.device == p.device
        assert lo <= h.data_ptr() and h.data_ptr() + 2 * h.numel() <= hi
        assert torch.equal(_bits(h), _bits(p.detach().to(torch.float16)))
    by_name = {names[id(p)]: h for p, h in copies.items()}
    H = CFG["hidden_size"]
    for tower in ("bert_q", "bert_c"):
        for i in range(CFG["num_hidden_layers"]):
            q, k, v = (by_name[f"{tower}.encoder.layer.{i}.attention.self.{n}.weight"] for n in ("query", "key", "value"))
            assert q.data_ptr() % 16 == 0
            assert k.data_ptr() == q.data_ptr() + 2 * H * H and v.data_ptr() == k.data_ptr() + 2 * H * H
        for n in ("attention.output.dense", "intermediate.dense", "output.dense"):
            assert by_name[f"{tower}.encoder.layer.0.{n}.weight"].data_ptr() % 16 == 0
        assert by_name[f"{tower}.pooler.dense.weight"].data_ptr() % 16 == 0
    assert by_name["proj_q.weight"].data_ptr() % 16 == 0 and by_name["proj_c.weight"].data_ptr() % 16 == 0


def test_training_with_the_copies_is_bit_identical(gpu_device):
    from proqa_amd.optim import FusedAdamW
    from proqa_amd.trainable import inbatch_loss
    sd = random_state_dict(CFG, seed=0)
    batches = [_on(gpu_device, oracle.small_batch(s)) for s in range(6)]
    runs = {}
    for use_copies in (False, True):
        model = _model(gpu_device, sd, freeze_words=True)
        params = [p for p in model.parameters() if p.requires_grad]
        kw = dict(half_copies=model.half_weights()) if use_copies else {}
        opt = FusedAdamW(params, lr=1e-3, max_grad_norm=2.0, loss_scale="dynamic", **kw)
        losses = []
        for step in range(3):
            for micro in range(2):
                out = model(batches[2 * step + micro])
                loss = inbatch_loss(out["q"], out["c"]) / 2
                losses.append(loss.detach())
                opt.scale_loss(loss).backward()
            opt.step()
            opt.zero_grad()
        assert int(opt.step_tensor) + int(opt.skipped_steps) == 3 and int(opt.step_tensor) >= 2
        runs[use_copies] = (torch.stack(losses).cpu(), {k: v.cpu() for k, v in model.state_dict().items()}, model)
    (loss_a, sd_a, _), (loss_b, sd_b, with_copies) = runs[False], runs[True]
    print("losses", loss_a.tolist(), loss_b.tolist())
    assert torch.equal(loss_a.view(torch.int32), loss_b.view(torch.int32))
    for k in sd_a:
        assert torch.equal(_bits(sd_a[k]), _bits(sd_b[k])), k
    assert any(not torch.equal(sd_a[k], sd[k]) for k in sd if "dense.weight" in k)
    # after three steps every copy is still its master's cast: the step wrote it
    for p, h in with_copies._half.copies.items():
        assert torch.equal(_bits(h), _bits(p.detach().to(torch.float16)))


def test_a_copy_never_goes_stale_silently(gpu_device):
    sd0, sd1 = random_state_dict(CFG, seed=0), random_state_dict(CFG, seed=1)
    batch = _on(gpu_device, oracle.small_batch(0))
    fresh1 = _forward_bits(_model(gpu_device, sd1), batch)
    assert not torch.equal(fresh1, _forward_bits(_model(gpu_device, sd0), batch))

    model = _model(gpu_device, sd0)
    model.half_weights()
    assert torch.equal(_forward_bits(model, batch), _forward_bits(_model(gpu_device, sd0), batch))
    model.load_state_dict(sd1)                                   # re-casts
    assert torch.equal(_forward_bits(model, batch), fresh1)

    model.load_state_dict(sd0)
    with torch.no_grad():                                        # an edit behind the module's back ...
        for k, p in model.named_parameters():
            p.copy_(sd1[k])
    assert not torch.equal(_forward_bits(model, batch), fresh1)  # (the matrices are still sd0's: that is what stale means)
    model.refresh_half_weights()                                 # ... and the public re-cast
    assert torch.equal(_forward_bits(model, batch), fresh1)

    assert model.to(gpu_device) is model and model._half is not None
    assert torch.equal(_forward_bits(model, batch), fresh1)
    # an _apply that moves the storage drops the copies: back to the per-forward casts, still right
    model._apply(lambda t: t.clone())
    assert model._half is None
    assert torch.equal(_forward_bits(model, batch), fresh1)
    model.refresh_half_weights()                                 # nothing to do, no error
    copies = model.half_weights()                                # and the copies can be taken again
    assert all(torch.equal(_bits(h), _bits(p.detach().half())) for p, h in copies.items())
    assert torch.equal(_forward_bits(model, batch), fresh1)


def test_half_copies_are_validated(gpu_device):
    from proqa_amd.optim import FusedAdamW
    p = torch.nn.Parameter(torch.zeros(8, 4, device=gpu_device))
    q = torch.nn.Parameter(torch.zeros(5, device=gpu_device))
    good = torch.zeros(8, 4, dtype=torch.float16, device=gpu_device)
    FusedAdamW([p, q], lr=1e-3, half_copies={p: good})
    FusedAdamW([p, q], lr=1e-3, half_copies={p: good.view(-1)})          # the same numel is enough
    with pytest.raises(ValueError, match="float16"):
        FusedAdamW([p, q], lr=1e-3, half_copies={p: torch.zeros(8, 4, dtype=torch.bfloat16, device=gpu_device)})
    with pytest.raises(ValueError, match="float16"):
        FusedAdamW([p, q], lr=1e-3, half_copies={p: torch.zeros(8, 4, device=gpu_device)})
    with pytest.raises(ValueError, match="elements"):
        FusedAdamW([p, q], lr=1e-3, half_copies={p: torch.zeros(8, 5, dtype=torch.float16, device=gpu_device)})
    with pytest.raises(ValueError, match="device"):
        FusedAdamW([p, q], lr=1e-3, half_copies={p: torch.zeros(8, 4, dtype=torch.float16)})
    with pytest.raises(ValueError, match="contiguous"):
        FusedAdamW([p, q], lr=1e-3, half_copies={p: torch.zeros(8, 8, dtype=torch.float16, device=gpu_device)[:, ::2]})
    with pytest.raises(ValueError, match="not a parameter"):
        FusedAdamW([q], lr=1e-3, half_copies={p: good})


def test_the_plain_step_writes_copies_too(gpu_device):
    from proqa_amd.optim import FusedAdamW
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(300, 70, device=gpu_device))
    h = torch.zeros(300, 70, dtype=torch.float16, device=gpu_device)
    opt = FusedAdamW([p], lr=1e-2, half_copies={p: h})
    assert opt.half_copies[p] is h
    p.grad = torch.randn(300, 70, device=gpu_device)
    before = p.detach().clone()
    opt.step()
    assert not torch.equal(p.detach(), before)
    assert torch.equal(_bits(h), _bits(p.detach().half()))
