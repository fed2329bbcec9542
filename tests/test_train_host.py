"""What of the trainable retriever can be checked without a GPU: the float64 / fp32 restatement the GPU tests compare against
(tests/train_oracle.py) equals the frozen fp32 oracle, trains on the fixed batch of tests/test_trainable_gpu.py, and the
module's parameter layout and refusals."""
import pytest
import torch

import train_oracle
from oracle import bert_torch_cpu
from proqa_amd.retriever import BertForRetriever, random_state_dict

CFG = train_oracle.SMALL_CONFIG
L, NH = CFG["num_hidden_layers"], CFG["num_attention_heads"]


@pytest.mark.parametrize("seed", [0, 1])
def test_restated_tower_equals_the_frozen_oracle(seed):
    sd = random_state_dict(CFG, seed=seed)
    batch = train_oracle.small_batch(seed)
    for is_q, ids, mask in ((True, batch["input_ids_q"], batch["input_mask_q"]), (False, batch["input_ids_c"], batch["input_mask_c"])):
        want = bert_torch_cpu.get_embed(sd, ids, mask, is_q, L, NH)
        got32 = train_oracle.tower_forward(sd, ids, mask, is_q, L, NH)
        got64 = train_oracle.tower_forward({k: v.double() for k, v in sd.items()}, ids, mask, is_q, L, NH)
        assert (got32 - want).abs().max() < 2e-5 and (got64 - want.double()).abs().max() < 2e-5
        # the fp16-storage mode stays within the forward tolerance of the GPU tests (tests/test_encoder_gpu.py TOL_GOLDEN)
        got16 = train_oracle.tower_forward(sd, ids, mask, is_q, L, NH, storage="fp16")
        assert (got16 - want).abs().max() < 1.5e-3


def test_restated_gradients_agree_between_float32_and_float64():
    sd = random_state_dict(CFG, seed=0)
    batch = train_oracle.small_batch(0)
    loss64, g64, _ = train_oracle.model_gradients(sd, batch, L, NH)
    loss32, g32, _ = train_oracle.model_gradients(sd, batch, L, NH, dtype=torch.float32)
    assert abs(loss64 - loss32) < 1e-5 and abs(loss64 - 2.08) < 0.05         # ln 8 = 2.079 at the start
    for k in g64:
        if g64[k].abs().max() < 1e-12:      # no gradient: the key bias (softmax-invariant), proj_c.bias (the rows of d_c sum to 0)
            assert k.endswith("key.bias") or k == "proj_c.bias"
            assert g32[k].abs().max() < 1e-6, k
        else:
            assert train_oracle.rel_err(g32[k], g64[k]) < 1e-4, k
    # structure: rows the batch does not touch have no gradient
    used = torch.unique(torch.cat([batch["input_ids_q"][batch["input_mask_q"]], ]))
    d_word = g64["bert_q.embeddings.word_embeddings.weight"]
    unused = torch.ones(CFG["vocab_size"], dtype=torch.bool)
    unused[used] = False
    assert (d_word[unused] == 0).all() and (d_word[used] != 0).any()
    assert (g64["bert_q.embeddings.token_type_embeddings.weight"][1] == 0).all()
    assert (g64["bert_q.encoder.layer.0.attention.self.key.bias"] == 0).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_twenty_steps_fit_the_fixed_batch_in_fp32(seed):
    """The training condition of tests/test_trainable_gpu.py, on the fp32 restatement: loss <= 0.2 and 8/8 after 20 steps."""
    trace = train_oracle.train_steps(random_state_dict(CFG, seed=seed), train_oracle.small_batch(seed), L, NH, steps=20)
    print(seed, "start", trace[0], "step 10", trace[10], "step 20", trace[20])
    assert abs(trace[0][0] - 2.08) < 0.05
    assert trace[20][0] <= 0.2 and trace[20][1] == 8


def test_state_dict_keys_are_the_reference_layout():
    from proqa_amd import trainable
    keys = trainable.state_dict_keys(CFG)
    ref = BertForRetriever.state_dict_keys(type("C", (), {"config": trainable.config_from_dict(CFG)})())
    assert keys == ref and len(keys) == len(set(keys))
    shapes = trainable._parameter_shapes(trainable.config_from_dict(CFG))
    want = random_state_dict(CFG)
    assert list(shapes) == keys and {k: tuple(v.shape) for k, v in want.items()} == shapes
    # the class itself: a torch.nn.Module whose parameters are created under these names
    assert issubclass(trainable.TrainableRetriever, torch.nn.Module)


def test_dropout_and_cpu_are_refused():
    from proqa_amd import trainable
    with pytest.raises(ValueError, match="dropout"):
        trainable.TrainableRetriever(CFG, device="cuda", dropout=0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        trainable.TrainableRetriever(CFG, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        trainable.TrainableRetriever(CFG, device=torch.device("cpu"), dropout=0.0)
