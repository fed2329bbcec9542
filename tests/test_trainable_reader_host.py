"""What of the trainable reader can be checked without a GPU: the oracle (tests/reader_train_oracle.py) against torch.autograd
and against the reference's own BertRetrieveQA over transformers' BERT (tests/golden/reader_train_golden.npz), the key
lists, the tolerance tables of the two GPU test files, the constructor's refusals and the pure host side of the new entry
point."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import reader_train_oracle as oracle
from proqa_amd.reader import random_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = oracle.SMALL_CONFIG
L, NH = CFG["num_hidden_layers"], CFG["num_attention_heads"]


# ---- the typed embedding oracle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,pattern", [((128, 5, 40), "segments"), ((128, 5, 40), "outside"), ((768, 5, 24), "one_type"),
                                           ((128, 1, 1), "all1"), ((128, 9, 12), "all0")])
def test_closed_form_typed_backward_is_autograd(shape, pattern):
    import test_embed_typed_backward_gpu as G
    c, closed = G.case(shape, pattern)
    auto = oracle.embed_typed_backward_autograd(**c)
    for k in G.OUTPUTS:
        assert closed[k].dtype == torch.float64 and oracle.rel_err(closed[k], auto[k]) <= 1e-12, k
    if pattern == "outside":          # ids outside their tables went to row 0
        assert closed["d_word"][0].abs().max() > 0 and closed["d_types"][0].abs().max() > 0


def test_typed_embedding_tolerance_table_is_reproduced():
    """Summation order inside torch's CPU kernels may move the figures a little between machines; the GPU test uses the
    recorded figures, this test says when they have drifted."""
    import test_embed_typed_backward_gpu as G
    worst = G.measure_reference_error()
    print({k: f"{v:.3e}" for k, v in worst.items()})
    assert set(worst) == set(G.REFERENCE_ERROR) == set(G.OUTPUTS)
    for k, recorded in G.REFERENCE_ERROR.items():
        assert worst[k] == pytest.approx(recorded, rel=0.25), (k, worst[k], recorded)
        assert f"{recorded:.3e}" in G.__doc__ and f"{4 * recorded:.3e}" in G.__doc__, k
        assert G.BOUNDS[k] == 4.0 * recorded


# ---- the reader oracle against the reference's class ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def float64_gradients(shared_norm=True):
    sd = random_state_dict(CFG, seed=0)
    return oracle.model_gradients(sd, oracle.SMALL_READER_BATCH, L, NH, shared_norm=shared_norm)


def test_oracle_agrees_with_the_reference_class():
    """reader_train_golden.npz: BertRetrieveQA.forward in train() and backward(), transformers' BertModel, float64
    (tests/golden/make_reader_train_golden.py).  1e-5 of max|ref| per tensor, the bar of reader_loss_golden."""
    from test_trainable_reader_gpu import CANCELS
    golden = np.load(os.path.join(HERE, "golden", "reader_train_golden.npz"))
    values, grads, _ = float64_gradients(True)
    assert abs(values["loss"] - float(golden["shared::loss"])) <= 1e-5 * abs(float(golden["shared::loss"]))
    other, _, _ = float64_gradients(False)
    assert abs(other["loss"] - float(golden["separate::loss"])) <= 1e-5 * abs(float(golden["separate::loss"]))
    seen = 0
    for key, g in grads.items():
        norm = float(golden[f"norm::{key}"])
        if f"full::{key}" in golden:
            want, got = torch.from_numpy(golden[f"full::{key}"]), g
        else:
            at = torch.from_numpy(golden[f"at::{key}"])
            want, got = torch.from_numpy(golden[f"values::{key}"]), g.reshape(-1)[at]
        if g.abs().max() == 0:
            # zero by construction here (unused towers, the pooler, key biases): the reference's is zero or rounding
            scale = max(float(golden[f"norm::{key.replace('key.bias', 'query.bias')}"]), 1e-300)
            assert norm <= 1e-9 * scale or norm == 0, (key, norm)
            continue
        if key in CANCELS:
            # zero in exact arithmetic; the reference rounds its logits to fp32 on the way (`.float()` around masked_fill)
            assert norm <= 1e-5 * float(golden[f"norm::{CANCELS[key][0]}"]), (key, norm)
            continue
        seen += 1
        assert abs(float(g.norm()) - norm) <= 1e-5 * norm, (key, float(g.norm()), norm)
        assert (got - want).abs().max().item() <= 1e-5 * max(want.abs().max().item(), g.abs().max().item()), key
    assert seen > 60
    types = torch.from_numpy(golden["full::bert.embeddings.token_type_embeddings.weight"])
    assert types.shape == (2, 128) and (types[0] != 0).any() and (types[1] != 0).any()


def test_state_dict_keys_are_the_reference_classes():
    from proqa_amd.trainable_reader import state_dict_keys
    with open(os.path.join(HERE, "golden", "reader_state_dict_keys.json")) as f:
        reference_keys = [k for k in json.load(f) if not k.endswith("position_ids")]
    ours = state_dict_keys(CFG)
    assert sorted(ours) == sorted(reference_keys) and len(set(ours)) == len(ours)
    assert sorted(ours) == sorted(random_state_dict(CFG, seed=0))
    assert state_dict_keys(dict(CFG)) == ours
    # the reference's order: bert, retriever, qa_outputs
    assert ours[0].startswith("bert.") and ours[-2:] == ["qa_outputs.weight", "qa_outputs.bias"]
    assert ours.index("retriever.bert_q.embeddings.word_embeddings.weight") > ours.index("bert.pooler.dense.bias")


# ---- the tolerance tables and the training figures of tests/test_trainable_reader_gpu.py ------------------------------------------

def test_reader_tolerance_tables_are_reproduced():
    import test_trainable_reader_gpu as G
    forward, worst = G.measure_reference_error()
    print({k: f"{v:.3e}" for k, v in forward.items()})
    print("\n".join(f"                  {k:<48} {v:.3e} / {4 * v:.3e}" for k, v in worst.items()))
    assert set(forward) == set(G.FORWARD_REFERENCE_ERROR)
    for k, recorded in G.FORWARD_REFERENCE_ERROR.items():
        assert forward[k] == pytest.approx(recorded, rel=0.25), (k, forward[k], recorded)
        assert f"{recorded:.3e}" in G.__doc__ and f"{4 * recorded:.3e}" in G.__doc__, k
    assert set(worst) == set(G.REFERENCE_ERROR)
    for k, recorded in G.REFERENCE_ERROR.items():
        assert worst[k] == pytest.approx(recorded, rel=0.25), (k, worst[k], recorded)
        assert f"{recorded:.3e}" in G.__doc__ and f"{4 * recorded:.3e}" in G.__doc__, k
        assert G.BOUNDS[k] == 4.0 * recorded
    # every parameter that is compared has a bound; what is left out is zero in float64
    _, grads, _ = float64_gradients(True)
    for key, g in grads.items():
        if G.zero_by_construction(key) or key.endswith("attention.self.key.bias"):
            assert g.abs().max() == 0, key
        elif key in G.CANCELS:
            sibling, bound_kind = G.CANCELS[key]
            assert g.abs().max() <= 1e-12 * grads[sibling].abs().max() and bound_kind in G.BOUNDS, key
        else:
            assert g.abs().max() > 0 and G.kind(key) in G.BOUNDS, key
    assert (grads["retriever.bert_q.embeddings.token_type_embeddings.weight"][1] == 0).all()
    assert all((grads["bert.embeddings.token_type_embeddings.weight"][r] != 0).any() for r in (0, 1))


def test_twenty_steps_of_the_float32_oracle():
    import test_trainable_reader_gpu as G
    trace = oracle.train_steps(random_state_dict(CFG, seed=0), oracle.SMALL_READER_BATCH, L, NH, steps=20)
    print("loss: start", trace[0], "after 20", trace[-1])
    assert abs(trace[0] - G.ORACLE_LOSS_START) <= 1e-3 and abs(trace[-1] - G.ORACLE_LOSS_AFTER_20) <= 0.02
    assert f"{G.ORACLE_LOSS_START:.4f}" in G.__doc__ and f"{G.ORACLE_LOSS_AFTER_20:.4f}" in G.__doc__
    assert trace[-1] < 0.1 * trace[0]


# ---- the module and the entry point, as far as they go without a GPU ---------------------------------------------------------------

def test_constructor_refusals():
    from proqa_amd.trainable_reader import TrainableReader
    with pytest.raises(ValueError, match="separate / add_select are not built"):
        TrainableReader(CFG, separate=True)
    with pytest.raises(ValueError, match="separate / add_select are not built"):
        TrainableReader(CFG, add_select=True)
    for name in ("qa_drop", "hidden_dropout_prob", "attention_probs_dropout_prob"):
        for rate in (-0.1, 0.95):
            with pytest.raises(ValueError, match=name):
                TrainableReader(CFG, **{name: rate})
    with pytest.raises(RuntimeError, match="no CPU path"):
        TrainableReader(CFG, device="cpu")
    args = type("Args", (), dict(shared_norm=True, drop_early=False, qa_drop=0.0, separate=True, add_select=False, retriever_path=""))()
    with pytest.raises(ValueError, match="not built"):
        TrainableReader.from_args(CFG, args)


def test_entry_point_refuses_before_the_device_is_touched():
    from proqa_amd import _lib
    lib = _lib.load()
    assert lib.proqa_abi_version() == 7
    typed, untyped = lib.proqa_embed_layernorm_typed_backward_workspace_bytes, lib.proqa_backward_workspace_bytes
    assert typed(768) == 512 * 4 * 768 * 4 and typed(0) == 0 and typed(-8) == 0
    assert untyped(768) == 512 * 3 * 768 * 4                    # what it returned before this operator existed
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)           # never dereferenced: every call below fails its host-side checks

    def call(batch=2, seq_len=8, hidden=128, n_types=2, ws_bytes=None, dy=p, type_ids=None, ws=p):
        return lib.proqa_embed_layernorm_typed_varlen_backward_f16(
            dy, p, type_ids, p, batch, seq_len, hidden, 16, p, 50, p, p, n_types, p, 1e-12, p, p, p, p, p, ws,
            typed(hidden) if ws_bytes is None else ws_bytes, None)

    for kw, word in ((dict(n_types=3), b"n_types"), (dict(n_types=0), b"n_types"), (dict(hidden=100), b"hidden"),
                     (dict(hidden=1032), b"hidden"), (dict(seq_len=513), b"seq_len"), (dict(ws_bytes=untyped(128)), b"workspace"),
                     (dict(dy=None), b"NULL"), (dict(ws=None), b"NULL")):
        assert call(**kw) == -1 and word in lib.proqa_last_error(), (kw, lib.proqa_last_error())
