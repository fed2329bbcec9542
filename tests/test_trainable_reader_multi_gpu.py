"""TrainableReader.forward on a LIST of the sampler's net_input dicts: several questions in one pass (one reader-tower pass,
one question-tower pass, one reader_loss_multi call), against tests/reader_train_oracle.py question by question.

Configuration: train_oracle.SMALL_CONFIG, proqa_amd.reader.random_state_dict weights (seed 0), and three questions derived
from reader_train_oracle.small_reader_batch (QUESTIONS below): the batch itself (5 sequences up to 40 tokens, 3 answer
slots, 40 passages); 2 sequences of 33 / 21 tokens with other token ids, 2 answer slots, a question of 5 tokens and 25
passages; and 1 sequence of 40 tokens with 7 passages.  The list route pads them on the device to 40 columns and 3 slots.

Tolerances (the project's rule: four times the error of the oracle's storage="fp16" mode against float64;
measure_reference_error(), CPU, reproduced by tests/test_trainable_reader_multi_host.py).  The float64 reference of the pass is
oracle.model_gradients per question, the gradients summed in float64; the fp16 mode is summed the same way.
  forward     |gpu - ref| / |ref| of every question's loss.  The error of one loss is one draw of the fp16 roundings (the three
              questions give 2.044e-05, 3.281e-06, 1.120e-05); the bound of every question is four times the LARGEST of the three,
              measured / allowed:
                  loss of a question                               2.044e-05 / 8.176e-05
  gradients   max|gpu - ref| / max|ref| of the three questions' summed gradient per parameter at loss scale 1024 (shared
              norm); one bound per KIND of parameter as in tests/test_trainable_reader_gpu.py, measured / allowed:
                  embeddings.word_embeddings.weight                1.381e-03 / 5.524e-03
                  embeddings.position_embeddings.weight            9.799e-04 / 3.920e-03
                  embeddings.token_type_embeddings.weight          1.063e-02 / 4.252e-02
                  embeddings.LayerNorm.weight                      1.236e-03 / 4.944e-03
                  embeddings.LayerNorm.bias                        9.555e-03 / 3.822e-02
                  encoder.layer.attention.self.query.weight        1.369e-03 / 5.476e-03
                  encoder.layer.attention.self.query.bias          2.364e-03 / 9.456e-03
                  encoder.layer.attention.self.key.weight          2.021e-03 / 8.084e-03
                  encoder.layer.attention.self.value.weight        5.244e-03 / 2.098e-02
                  encoder.layer.attention.self.value.bias          9.067e-03 / 3.627e-02
                  encoder.layer.attention.output.dense.weight      7.772e-03 / 3.109e-02
                  encoder.layer.attention.output.dense.bias        1.112e-02 / 4.448e-02
                  encoder.layer.attention.output.LayerNorm.weight  1.581e-03 / 6.324e-03
                  encoder.layer.attention.output.LayerNorm.bias    1.041e-02 / 4.164e-02
                  encoder.layer.intermediate.dense.weight          1.736e-03 / 6.944e-03
                  encoder.layer.intermediate.dense.bias            2.059e-03 / 8.236e-03
                  encoder.layer.output.dense.weight                2.240e-03 / 8.960e-03
                  encoder.layer.output.dense.bias                  1.271e-02 / 5.084e-02
                  encoder.layer.output.LayerNorm.weight            1.761e-03 / 7.044e-03
                  encoder.layer.output.LayerNorm.bias              1.359e-02 / 5.436e-02
                  pooler.dense.weight                              1.212e-03 / 4.848e-03
                  pooler.dense.bias                                4.836e-04 / 1.934e-03
                  proj.weight                                      6.504e-04 / 2.602e-03
                  proj.bias                                        1.961e-04 / 7.844e-04
                  qa_outputs.weight                                9.756e-04 / 3.902e-03
  The parameters whose float64 gradient is zero by construction, and the two that cancel, are those of
  tests/test_trainable_reader_gpu.py (sums of zeros are zero) and are handled by its rules.
"""
import functools

import pytest
import torch

import reader_train_oracle as oracle
from proqa_amd.reader import random_state_dict
from test_trainable_reader_gpu import CANCELS, CFG, L, LOSS_SCALE, NH, kind, make_model, on, zero_by_construction

pytestmark = pytest.mark.gpu

FORWARD_REFERENCE_ERROR = [2.044e-05, 3.281e-06, 1.120e-05]          # per question; the bound takes the largest
REFERENCE_ERROR = {
    "embeddings.word_embeddings.weight": 1.381e-03,
    "embeddings.position_embeddings.weight": 9.799e-04,
    "embeddings.token_type_embeddings.weight": 1.063e-02,
    "embeddings.LayerNorm.weight": 1.236e-03,
    "embeddings.LayerNorm.bias": 9.555e-03,
    "encoder.layer.attention.self.query.weight": 1.369e-03,
    "encoder.layer.attention.self.query.bias": 2.364e-03,
    "encoder.layer.attention.self.key.weight": 2.021e-03,
    "encoder.layer.attention.self.value.weight": 5.244e-03,
    "encoder.layer.attention.self.value.bias": 9.067e-03,
    "encoder.layer.attention.output.dense.weight": 7.772e-03,
    "encoder.layer.attention.output.dense.bias": 1.112e-02,
    "encoder.layer.attention.output.LayerNorm.weight": 1.581e-03,
    "encoder.layer.attention.output.LayerNorm.bias": 1.041e-02,
    "encoder.layer.intermediate.dense.weight": 1.736e-03,
    "encoder.layer.intermediate.dense.bias": 2.059e-03,
    "encoder.layer.output.dense.weight": 2.240e-03,
    "encoder.layer.output.dense.bias": 1.271e-02,
    "encoder.layer.output.LayerNorm.weight": 1.761e-03,
    "encoder.layer.output.LayerNorm.bias": 1.359e-02,
    "pooler.dense.weight": 1.212e-03,
    "pooler.dense.bias": 4.836e-04,
    "proj.weight": 6.504e-04,
    "proj.bias": 1.961e-04,
    "qa_outputs.weight": 9.756e-04,
}
FORWARD_BOUND = 4.0 * max(FORWARD_REFERENCE_ERROR)
BOUNDS = {k: 4.0 * v for k, v in REFERENCE_ERROR.items()}


def _rows(batch, rows, width, n_answers, n_paras, q_tokens):
    """`rows` of a small_reader_batch, cut to `width` columns, `n_answers` slots, `n_paras` passages and q_tokens question
    tokens"""
    out = {k: batch[k][rows, :width].clone() for k in ("input_ids", "input_mask", "segment_ids", "paragraph_mask")}
    out["input_ids_q"] = (batch["input_ids_q"][rows, :q_tokens + 1] * (torch.arange(q_tokens + 1)[None] < q_tokens)).clone()
    out["input_mask_q"] = (torch.arange(q_tokens + 1)[None] < q_tokens).expand(len(rows), q_tokens + 1).contiguous()
    out["para_embed"] = batch["para_embed"][:n_paras].clone()
    out["top5000_labels"] = batch["top5000_labels"][:n_paras].clone()
    out["start_positions"] = batch["start_positions"][rows, :n_answers].clone()
    out["end_positions"] = batch["end_positions"][rows, :n_answers].clone()
    out["para_targets"] = out["top5000_labels"][:len(rows)].clone()
    return out


@functools.lru_cache(maxsize=None)
def questions():
    q0 = oracle.SMALL_READER_BATCH
    q1 = _rows(oracle.small_reader_batch(1), [1, 2], 33, 2, 25, 5)          # 33 and 21 tokens
    q1["start_positions"], q1["end_positions"] = torch.tensor([[6, 20], [8, -1]]), torch.tensor([[10, 31], [12, -1]])
    q2 = _rows(oracle.small_reader_batch(2), [0], 40, 3, 7, 6)              # one sequence of 40 tokens
    q2["start_positions"], q2["end_positions"] = torch.tensor([[30, 9, -1]]), torch.tensor([[33, 9, -1]])
    q2["top5000_labels"] = torch.zeros(7, dtype=torch.long)
    q2["top5000_labels"][3] = 1
    return [q0, q1, q2]


@functools.lru_cache(maxsize=None)
def reference():
    """(state dict, [float64 loss per question], float64 gradients summed over the questions) -- computed once"""
    sd = random_state_dict(CFG, seed=0)
    losses, total = [], None
    for batch in questions():
        values, grads, _ = oracle.model_gradients(sd, batch, L, NH, shared_norm=True)
        losses.append(values["loss"])
        total = grads if total is None else {k: total[k] + grads[k] for k in total}
    return sd, losses, total


def measure_reference_error():
    """([relative error of each question's loss], {kind: rel_err of the summed gradient}) of the storage='fp16' oracle at
    loss scale 1024 against float64 -- CPU only; the tables in the header are its output."""
    sd, ref_losses, ref = reference()
    forward, total = [], None
    for batch, want in zip(questions(), ref_losses):
        values, got, _ = oracle.model_gradients(sd, batch, L, NH, shared_norm=True, dtype=torch.float32, storage="fp16",
                                                loss_scale=LOSS_SCALE)
        forward.append(abs(values["loss"] - want) / abs(want))
        total = {k: v.double() for k, v in got.items()} if total is None else {k: total[k] + got[k].double() for k in total}
    worst = {}
    for k in ref:
        if ref[k].abs().max() > 0 and k not in CANCELS:
            worst[kind(k)] = max(worst.get(kind(k), 0.0), oracle.rel_err(total[k], ref[k]))
    return forward, worst


def gradients(model, net_input, scale=LOSS_SCALE):
    model.zero_grad(set_to_none=True)
    out = model(net_input)
    (out["loss"] * scale).backward()
    return out, {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def same_gradient_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def composed_by_hand(model, x, scale=LOSS_SCALE):
    """One question through the pieces a pass is made of, put together here and not by the module: run_tower for the reader
    tower, run_tower on row 0 of the question inputs, reader_loss through the single-question C entry; the dropout triple is
    read from model.dropout_state() and the state is left as it is.  -> (reader_loss's dict, the parameters' gradients)"""
    from proqa_amd.reader_loss import reader_loss
    from proqa_amd.trainable import run_tower
    from proqa_amd.trainable_reader import _PARAGRAPH_MESSAGE, _paragraph_geometry
    model.zero_grad(set_to_none=True)
    seed, call = model.dropout_state()
    p_hid, p_att = model.hidden_dropout_prob, model.attention_probs_dropout_prob
    pmask = x["paragraph_mask"].to(torch.bool)
    geometry = {}

    def paragraph_probe(lens):
        geometry["para_offset"], bad = _paragraph_geometry(pmask, lens)
        return bad, _PARAGRAPH_MESSAGE

    hidden, cu, _, max_len = run_tower(model._flat, "bert", model.config, x["input_ids"], x["input_mask"],
                                       type_ids=x["segment_ids"], drop=(p_hid, p_att, seed, call), probe_extra=paragraph_probe,
                                       deterministic=model.deterministic)
    q = run_tower(model.retriever._flat, "bert_q", model.config, x["input_ids_q"][:1], x["input_mask_q"][:1], proj="proj_q",
                  drop=(p_hid, p_att, seed, (call + 1) & 0xFFFFFF), deterministic=model.deterministic)
    out = reader_loss(hidden, model._flat["qa_outputs.weight"], model._flat["qa_outputs.bias"], q, x["para_embed"],
                      x["top5000_labels"], x["start_positions"], x["end_positions"], geometry["para_offset"], cu_seqlens=cu,
                      shared_norm=model.shared_norm, early=not model.drop_early, qa_drop=model.qa_drop,
                      dropout_state=(seed, (call + 2) & 0xFFFFFF), max_seq_len=max_len)
    (out["loss"] * scale).backward()
    return out, {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def test_a_list_of_one_question_is_the_dict_route(gpu_device):
    """model(dict), model([dict]) and model((dict,)) against the single-question route composed by hand, bit for bit; once
    without dropout, once with all three rates set (the head's mask coordinate on a pack of one is the question's own row)."""
    from proqa_amd.trainable_reader import CALLS_PER_FORWARD
    sd, *_ = reference()
    for rates in ({}, dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, qa_drop=0.1)):
        model = make_model(gpu_device, sd, deterministic=True, dropout_seed=11, **rates)
        for batch in questions():
            dev_batch = on(gpu_device, batch)
            state = model.dropout_state()
            want, grads_want = composed_by_hand(model, dev_batch)
            assert model.dropout_state() == state
            for net_input in (dev_batch, [dev_batch], (dev_batch,)):
                model.set_dropout_state(state)
                got, grads = gradients(model, net_input)
                assert model.dropout_state() == (state[0], state[1] + (CALLS_PER_FORWARD if rates else 0))
                if isinstance(net_input, dict):
                    assert set(got) == {"loss", "joint", "early"} and all(got[k].dim() == 0 for k in got)
                else:
                    assert set(got) == {"loss", "losses", "joint", "early"} and got["losses"].shape == (1,)
                    assert torch.equal(got["losses"].detach().view(torch.int32), got["loss"].detach().reshape(1).view(torch.int32))
                assert got["loss"].dim() == 0 and got["loss"].requires_grad and not got["joint"].requires_grad
                for k in ("loss", "joint", "early"):
                    assert torch.equal(want[k].detach().reshape(1).view(torch.int32),
                                       got[k].detach().reshape(1).view(torch.int32)), (k, rates)
                same_gradient_bits(grads_want, grads)
        if rates:       # the masks were really drawn: another call gives another loss
            other, _ = gradients(model, dev_batch)
            assert other["loss"].item() != want["loss"].item()


def test_three_questions_match_float64(gpu_device):
    sd, ref_losses, ref = reference()
    model = make_model(gpu_device, sd)
    out, grads = gradients(model, [on(gpu_device, b) for b in questions()])
    assert out["losses"].shape == (3,) and out["joint"].shape == (3,) and out["early"].shape == (3,)
    assert out["loss"].item() == pytest.approx(out["losses"].sum().item(), rel=1e-6)
    for i, want in enumerate(ref_losses):
        err = abs(out["losses"][i].item() - want) / abs(want)
        print(f"question {i} loss: gpu {out['losses'][i].item():.6f} float64 {want:.6f} error {err:.3e} bound {FORWARD_BOUND:.3e}")
        assert err <= FORWARD_BOUND, (i, err)
        # and it is the loss of the question alone, to the bit
        assert model(on(gpu_device, questions()[i]))["loss"].item() == out["losses"][i].item()
    failures = []
    for k, want in ref.items():
        if zero_by_construction(k):
            assert want.abs().max() == 0 and grads[k] is None, k
            continue
        assert grads[k] is not None and grads[k].dtype == torch.float32, k
        got = grads[k].cpu().double() / LOSS_SCALE
        if k.endswith("attention.self.key.bias"):
            assert want.abs().max() == 0
            layer = k[:-len("key.bias")]
            scale = max(ref[layer + "query.bias"].abs().max().item(), ref[layer + "value.bias"].abs().max().item())
            err, bound = got.abs().max().item() / scale, max(BOUNDS[kind(layer + "query.bias")], BOUNDS[kind(layer + "value.bias")])
        elif k in CANCELS:
            sibling, bound_kind = CANCELS[k]
            assert want.abs().max() <= 1e-12 * ref[sibling].abs().max()
            err, bound = got.abs().max().item() / ref[sibling].abs().max().item(), BOUNDS[bound_kind]
        else:
            err, bound = oracle.rel_err(got, want), BOUNDS[kind(k)]
        print(f"{k}: error {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            failures.append((k, err, bound))
    assert not failures, failures
    q_types = grads["retriever.bert_q.embeddings.token_type_embeddings.weight"]
    assert (q_types[1] == 0).all() and (q_types[0] != 0).any()


def test_dropout_masks_are_a_function_of_the_state(gpu_device):
    from proqa_amd.trainable_reader import CALLS_PER_FORWARD
    sd, *_ = reference()
    batches = [on(gpu_device, b) for b in questions()]
    rates = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, qa_drop=0.1)
    model = make_model(gpu_device, sd, dropout_seed=11, deterministic=True, **rates)
    out_a, grads_a = gradients(model, batches)
    assert model.dropout_state() == (11, CALLS_PER_FORWARD)          # one triple per PASS, not per question
    model.set_dropout_state((11, 0))
    out_b, grads_b = gradients(model, batches)
    assert torch.equal(out_a["losses"], out_b["losses"])
    same_gradient_bits(grads_a, grads_b)
    out_c, _ = gradients(model, batches)                             # state (11, 3): other masks
    assert model.dropout_state() == (11, 2 * CALLS_PER_FORWARD)
    assert all(out_c["losses"][i].item() != out_a["losses"][i].item() for i in range(3))
    plain = make_model(gpu_device, sd, deterministic=True)
    out_p, _ = gradients(plain, batches)
    assert plain.dropout_state()[1] == 0 and all(out_p["losses"][i].item() != out_a["losses"][i].item() for i in range(3))


def test_refusals(gpu_device):
    sd, *_ = reference()
    model = make_model(gpu_device, sd)
    batches = [on(gpu_device, b) for b in questions()]
    with pytest.raises(ValueError, match="empty list"):
        model([])
    model.eval()
    with pytest.raises(ValueError, match="training pass"):
        model(batches)
    with torch.no_grad():
        assert set(model(batches[0])) == {"start_logits", "end_logits", "rank_logits"}       # a dict in eval(): today's route
    model.train()
    hole = dict(batches[1], paragraph_mask=batches[1]["paragraph_mask"].clone())
    hole["paragraph_mask"][0, 10] = 0
    with pytest.raises(ValueError, match="paragraph_mask"):
        model([batches[0], hole])
