"""proqa_amd.trainable.TrainableRetriever on the GPU against tests/train_oracle.py: forward, every parameter's gradient,
20 optimizer steps, the checkpoint round trip into the inference class, and a GradScaler overflow.

Configuration: hidden 128, 2 layers, 2 heads, intermediate 512, vocabulary 120, 64 positions, random_state_dict weights
(seed 0), 8 pairs (questions of 3-12 tokens, paragraphs of 5-40): train_oracle.SMALL_CONFIG / small_batch.

Tolerances
  forward     TOL_GOLDEN of tests/test_encoder_gpu.py (what get_embed of a 2-layer model is held to).
  gradients   max|gpu - ref| / max|ref| per parameter against float64, at loss scale 1024; the bound is four times the same
              measure of the oracle's storage="fp16" mode (measure_reference_error(), CPU), as in
              tests/test_train_ops_gpu.py.  One bound per KIND of parameter (the maximum over the parameters of the kind
              and both towers), measured / allowed:
                  embeddings.word_embeddings.weight                2.062e-03 / 8.248e-03
                  embeddings.position_embeddings.weight            8.241e-03 / 3.296e-02
                  embeddings.token_type_embeddings.weight          8.676e-03 / 3.470e-02
                  embeddings.LayerNorm.weight                      2.096e-03 / 8.384e-03
                  embeddings.LayerNorm.bias                        8.581e-03 / 3.432e-02
                  encoder.layer.attention.self.query.weight        2.606e-03 / 1.042e-02
                  encoder.layer.attention.self.query.bias          2.840e-03 / 1.136e-02
                  encoder.layer.attention.self.key.weight          3.381e-03 / 1.352e-02
                  encoder.layer.attention.self.value.weight        4.671e-03 / 1.868e-02
                  encoder.layer.attention.self.value.bias          9.146e-03 / 3.658e-02
                  encoder.layer.attention.output.dense.weight      4.654e-03 / 1.862e-02
                  encoder.layer.attention.output.dense.bias        8.187e-03 / 3.275e-02
                  encoder.layer.attention.output.LayerNorm.weight  2.345e-03 / 9.380e-03
                  encoder.layer.attention.output.LayerNorm.bias    7.985e-03 / 3.194e-02
                  encoder.layer.intermediate.dense.weight          4.009e-03 / 1.604e-02
                  encoder.layer.intermediate.dense.bias            4.305e-03 / 1.722e-02
                  encoder.layer.output.dense.weight                2.346e-03 / 9.384e-03
                  encoder.layer.output.dense.bias                  7.541e-03 / 3.016e-02
                  encoder.layer.output.LayerNorm.weight            2.511e-03 / 1.004e-02
                  encoder.layer.output.LayerNorm.bias              9.320e-03 / 3.728e-02
                  pooler.dense.weight                              1.853e-03 / 7.412e-03
                  pooler.dense.bias                                5.701e-03 / 2.280e-02
                  proj.weight                                      2.030e-03 / 8.120e-03
                  proj.bias                                        2.339e-02 / 9.356e-02
              The key bias has no gradient (exactly zero in the oracle): the module's is held to the bound of the biases
              relative to the query / value bias gradients of its layer.  Neither has proj_c.bias (the rows of
              softmax - one-hot sum to zero, so sum_i d_c[i] = 0): held to the proj.bias bound relative to the gradient of
              proj_q.bias.
  training    loss <= 0.2 (a tenth of ln 8) and 8/8 after 20 steps: the fp32 restatement reaches <= 2.2e-4
              (tests/test_train_host.py), which leaves three orders of magnitude for fp16.
"""
import functools

import pytest
import torch

import train_oracle as oracle
from proqa_amd.retriever import random_state_dict

pytestmark = pytest.mark.gpu

CFG = oracle.SMALL_CONFIG
L, NH = CFG["num_hidden_layers"], CFG["num_attention_heads"]
LOSS_SCALE = 1024.0

REFERENCE_ERROR = {
    "embeddings.word_embeddings.weight": 2.062e-03,
    "embeddings.position_embeddings.weight": 8.241e-03,
    "embeddings.token_type_embeddings.weight": 8.676e-03,
    "embeddings.LayerNorm.weight": 2.096e-03,
    "embeddings.LayerNorm.bias": 8.581e-03,
    "encoder.layer.attention.self.query.weight": 2.606e-03,
    "encoder.layer.attention.self.query.bias": 2.840e-03,
    "encoder.layer.attention.self.key.weight": 3.381e-03,
    "encoder.layer.attention.self.value.weight": 4.671e-03,
    "encoder.layer.attention.self.value.bias": 9.146e-03,
    "encoder.layer.attention.output.dense.weight": 4.654e-03,
    "encoder.layer.attention.output.dense.bias": 8.187e-03,
    "encoder.layer.attention.output.LayerNorm.weight": 2.345e-03,
    "encoder.layer.attention.output.LayerNorm.bias": 7.985e-03,
    "encoder.layer.intermediate.dense.weight": 4.009e-03,
    "encoder.layer.intermediate.dense.bias": 4.305e-03,
    "encoder.layer.output.dense.weight": 2.346e-03,
    "encoder.layer.output.dense.bias": 7.541e-03,
    "encoder.layer.output.LayerNorm.weight": 2.511e-03,
    "encoder.layer.output.LayerNorm.bias": 9.320e-03,
    "pooler.dense.weight": 1.853e-03,
    "pooler.dense.bias": 5.701e-03,
    "proj.weight": 2.030e-03,
    "proj.bias": 2.339e-02,
}
BOUNDS = {k: 4.0 * v for k, v in REFERENCE_ERROR.items()}


def kind(key):
    """the kind of a parameter: its name without the tower and the layer number"""
    parts = [p for p in key.split(".") if not p.isdigit()]
    if parts[0].startswith("proj_"):
        return "proj." + parts[-1]
    return ".".join(parts[1:])


@functools.lru_cache(maxsize=None)
def reference():
    """(state dict, CPU batch, float64 loss, float64 gradients, float64 outputs) -- computed once"""
    sd = random_state_dict(CFG, seed=0)
    batch = oracle.small_batch(0)
    loss, grads, out = oracle.model_gradients(sd, batch, L, NH)
    return sd, batch, loss, grads, out


def measure_reference_error():
    """{kind: max over its parameters of rel_err(storage='fp16' oracle at loss scale 1024, float64 oracle)} -- CPU only"""
    sd, batch, _, ref, _ = reference()
    _, got, _ = oracle.model_gradients(sd, batch, L, NH, dtype=torch.float32, storage="fp16", loss_scale=LOSS_SCALE)
    worst = {}
    for k in ref:
        if ref[k].abs().max() > 1e-12:
            worst[kind(k)] = max(worst.get(kind(k), 0.0), oracle.rel_err(got[k], ref[k]))
    return worst


def on(dev, batch):
    return {k: v.to(dev) for k, v in batch.items()}


def make_model(dev, sd):
    from proqa_amd.trainable import TrainableRetriever
    model = TrainableRetriever(CFG, device=dev)
    model.load_state_dict({"module." + k: v for k, v in sd.items()})       # the DataParallel prefix of a reference checkpoint
    return model


def test_module_surface(gpu_device):
    from proqa_amd.trainable import TrainableRetriever
    sd, batch, *_ = reference()
    model = make_model(gpu_device, sd)
    assert isinstance(model, torch.nn.Module)
    assert list(model.state_dict()) == model.state_dict_keys() == list(sd)
    assert all(p.dtype == torch.float32 and p.is_cuda and p.requires_grad for p in model.parameters())
    assert all(torch.equal(model.state_dict()[k].cpu(), v) for k, v in sd.items())
    model.load_state_dict(dict(sd, **{"bert_q.embeddings.position_ids": torch.arange(64)[None]}))      # newer transformers
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: v for k, v in sd.items() if k != "proj_q.bias"})
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.to("cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.cpu()
    with pytest.raises(RuntimeError, match="fp32 masters"):
        model.half()
    with pytest.raises(ValueError, match="dropout"):
        TrainableRetriever(CFG, device=gpu_device, dropout=0.1)
    bad = on(gpu_device, batch)
    bad["input_mask_q"] = bad["input_mask_q"].clone()
    bad["input_mask_q"][0, :2] = torch.tensor([False, True], device=gpu_device)
    with pytest.raises(ValueError, match="right-padded"):
        model(bad)


def test_forward_matches_the_oracle(gpu_device):
    from test_encoder_gpu import TOL_GOLDEN
    sd, batch, _, _, want = reference()
    model = make_model(gpu_device, sd)
    out = model(on(gpu_device, batch))
    assert set(out) == {"q", "c"}
    for k in ("q", "c"):
        assert out[k].shape == (8, 128) and out[k].dtype == torch.float16 and out[k].requires_grad
        err = (out[k].detach().cpu().double() - want[k]).abs().max().item()
        print(k, "max abs error", err)
        assert err < TOL_GOLDEN
    with torch.no_grad():
        emb = model.get_embed({"input_ids": batch["input_ids_c"].to(gpu_device), "input_mask": batch["input_mask_c"].to(gpu_device)},
                              False)["embed"]
    assert not emb.requires_grad and torch.equal(emb.view(torch.int16), out["c"].detach().view(torch.int16))


def test_every_parameter_gradient_matches_float64(gpu_device):
    from proqa_amd.trainable import inbatch_loss
    sd, batch, want_loss, ref, _ = reference()
    model = make_model(gpu_device, sd)
    out = model(on(gpu_device, batch))
    loss = inbatch_loss(out["q"], out["c"])
    assert loss.dtype == torch.float32 and abs(loss.item() - want_loss) < 2e-3
    (loss * LOSS_SCALE).backward()
    grads = {k: p.grad.detach().cpu().double() / LOSS_SCALE for k, p in model.named_parameters()}
    assert all(p.grad.dtype == torch.float32 for p in model.parameters())
    failures = []
    for k, want in ref.items():
        if k.endswith("attention.self.key.bias"):
            assert want.abs().max() == 0
            layer = k[:-len("key.bias")]
            scale = max(ref[layer + "query.bias"].abs().max().item(), ref[layer + "value.bias"].abs().max().item())
            err, bound = grads[k].abs().max().item() / scale, max(BOUNDS[kind(layer + "query.bias")], BOUNDS[kind(layer + "value.bias")])
        elif k == "proj_c.bias":
            assert want.abs().max() < 1e-12
            err, bound = grads[k].abs().max().item() / ref["proj_q.bias"].abs().max().item(), BOUNDS["proj.bias"]
        else:
            err, bound = oracle.rel_err(grads[k], want), BOUNDS[kind(k)]
        print(f"{k}: error {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            failures.append((k, err, bound))
    assert not failures, failures
    # structure: word rows not in the batch, position rows past the longest sequence, token-type row 1 are exactly zero
    for tower, side in (("bert_q", "q"), ("bert_c", "c")):
        ids, mask = batch[f"input_ids_{side}"], batch[f"input_mask_{side}"]
        unused = torch.ones(CFG["vocab_size"], dtype=torch.bool)
        unused[torch.unique(ids[mask])] = False
        g = {n: model.state_dict(keep_vars=True)[f"{tower}.embeddings.{n}.weight"].grad.cpu()
             for n in ("word_embeddings", "position_embeddings", "token_type_embeddings")}
        assert unused.any() and (g["word_embeddings"][unused] == 0).all() and (g["word_embeddings"][~unused] != 0).any()
        longest = int(mask.sum(1).max())
        assert (g["position_embeddings"][longest:] == 0).all() and (g["position_embeddings"][:longest] != 0).any()
        assert (g["token_type_embeddings"][1] == 0).all() and (g["token_type_embeddings"][0] != 0).any()


def in_batch_accuracy(q, c):
    from proqa_amd.inbatch import inbatch_eval
    out = inbatch_eval(q, c)
    return int((out["argmax"].cpu() == torch.arange(q.shape[0], dtype=torch.int32)).sum())


def test_twenty_steps_then_the_checkpoint_serves_inference(gpu_device, tmp_path):
    from test_encoder_gpu import TOL_GOLDEN
    from proqa_amd.retriever import BertForRetriever
    from proqa_amd.trainable import inbatch_loss
    sd, batch, *_ = reference()
    model = make_model(gpu_device, sd)
    dev_batch = on(gpu_device, batch)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, eps=1e-8, weight_decay=0.0)
    losses = []
    for _ in range(20):
        out = model(dev_batch)
        loss = inbatch_loss(out["q"], out["c"])
        losses.append(loss.item())
        opt.zero_grad()
        (loss * LOSS_SCALE).backward()
        for p in model.parameters():
            p.grad.div_(LOSS_SCALE)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 2.0)
        opt.step()
    with torch.no_grad():
        out = model(dev_batch)
        final = inbatch_loss(out["q"], out["c"]).item()
    print("loss: start", losses[0], "step 10", losses[10], "after 20", final)
    assert abs(losses[0] - 2.08) < 0.05
    assert final <= 0.2 and in_batch_accuracy(out["q"], out["c"]) == 8

    # the checkpoint, as the reference saves it, into the inference class
    path = tmp_path / "checkpoint_best.pt"
    torch.save(model.state_dict(), path)
    loaded = torch.load(path, map_location="cpu")
    assert list(loaded) == list(sd) and all(v.dtype == torch.float32 for v in loaded.values())
    infer = BertForRetriever(CFG, device=gpu_device)
    infer.load_state_dict(loaded)
    emb = {"q": infer.get_embed({"input_ids": dev_batch["input_ids_q"], "input_mask": dev_batch["input_mask_q"]}, True)["embed"],
           "c": infer.get_embed({"input_ids": dev_batch["input_ids_c"], "input_mask": dev_batch["input_mask_c"]}, False)["embed"]}
    for k in ("q", "c"):
        err = (emb[k].float() - out[k].float()).abs().max().item()
        print(k, "inference class against the module:", err)
        assert err < TOL_GOLDEN
    assert in_batch_accuracy(emb["q"], emb["c"]) == 8


def test_grad_scaler_skips_an_overflowing_step(gpu_device):
    from proqa_amd.trainable import inbatch_loss
    sd, batch, *_ = reference()
    model = make_model(gpu_device, sd)
    dev_batch = on(gpu_device, batch)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, eps=1e-8, weight_decay=0.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40, backoff_factor=2.0 ** -30, growth_interval=1000)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for step in range(2):
        out = model(dev_batch)
        loss = inbatch_loss(out["q"], out["c"])
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 2.0)
        scaler.step(opt)
        scaler.update()
        torch.cuda.synchronize()
        changed = any(not torch.equal(before[k], v) for k, v in model.state_dict().items())
        if step == 0:           # 2^40: the fp16 gradients overflow, the step is skipped, the scale backs off to 2^10
            assert not changed and scaler.get_scale() == 2.0 ** 10
        else:
            assert changed and all(torch.isfinite(v).all() for v in model.state_dict().values())
