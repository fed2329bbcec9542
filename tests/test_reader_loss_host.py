"""The reader's training objective without a GPU: the float64 restatement against the reference's own
BertRetrieveQA.forward (tests/golden/reader_loss_golden.npz, written by tests/golden/make_reader_loss_golden.py), its closed
forms against autograd, the C ABI's refusals, and the error table the GPU test's bounds come from."""
import ctypes
import os

import numpy as np
import pytest
import torch

import reader_loss_oracle as oracle
import test_reader_loss_gpu as G

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reader_loss_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("kind", ["both", "answers", "gold"])
@pytest.mark.parametrize("norm", ["shared", "separate"])
def test_oracle_matches_the_reference(golden, norm, kind):
    """within 1e-5 of max|ref| per tensor (the reference's float32 round trips leave 6e-9 in the loss, 1.4e-6 in the gradients)"""
    t = {k: torch.from_numpy(golden[k]) for k in ("hidden", "qa_w", "qa_b", "q", "para")}
    name = f"{norm}_{kind}"
    got = oracle.evaluate(t["hidden"], t["qa_w"], t["qa_b"], t["q"][0], t["para"], torch.from_numpy(golden[f"{name}::labels"]),
                          torch.from_numpy(golden[f"{name}::start"]), torch.from_numpy(golden[f"{name}::end"]),
                          golden["lens"].tolist(), golden["para_offset"].tolist(), shared_norm=norm == "shared")
    ref_loss = float(golden[f"{name}::loss"])
    assert ref_loss > 1.0 and abs(float(got["loss"]) - ref_loss) <= 1e-5 * abs(ref_loss)
    d_q = torch.from_numpy(golden[f"{name}::d_q"])
    assert (d_q[1:] == 0).all()                      # only q[0] carries a gradient in the reference
    for k, ref in (("d_hidden", torch.from_numpy(golden[f"{name}::d_hidden"])), ("d_q", d_q[0]),
                   ("d_qa_w", torch.from_numpy(golden[f"{name}::d_qa_w"])), ("d_qa_b", torch.from_numpy(golden[f"{name}::d_qa_b"]))):
        top = float(ref.abs().max())
        if top == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
        elif k == "d_qa_b":
            # the loss does not change when a constant is added to every start (end) logit: the bias gradient is zero by
            # cancellation, the reference's value is the noise of its float32 round trips; relative to the terms (size 1)
            assert top < 1e-6 and float((got[k] - ref).abs().max()) <= 1e-5, k
        else:
            assert float((got[k] - ref).abs().max()) <= 1e-5 * top, k


@pytest.mark.parametrize("shared_norm,early", G.VARIANTS)
@pytest.mark.parametrize("name", ["ragged128", "onerow", "dropout", "logits40"])
def test_closed_forms_equal_autograd(name, shared_norm, early):
    c = G.make_case(name)
    ref, auto = G.reference(name, shared_norm, early), oracle.autograd(**c, shared_norm=shared_norm, early=early)
    assert abs(float(ref["loss"]) - float(auto["loss"])) <= 1e-12 * max(1.0, abs(float(auto["loss"])))
    for k in ("d_hidden", "d_qa_w", "d_qa_b", "d_q"):
        scale = max(float(auto[k].abs().max()), 1.0)
        assert float((ref[k] - auto[k]).abs().max()) <= 1e-12 * scale, k


def test_degenerate_losses_are_zero():
    c = G.make_case("ragged128")
    none = torch.full_like(c["start"], -1)
    out = oracle.evaluate(**dict(c, start=none, end=none, labels=torch.zeros_like(c["labels"])))
    assert float(out["loss"]) == 0.0 and all(float(out[k].abs().max()) == 0.0 for k in ("d_hidden", "d_qa_w", "d_qa_b", "d_q"))
    assert float(oracle.evaluate(**c, early=False)["early"]) == 0.0


def test_abi_refuses_bad_sizes_without_a_gpu():
    from proqa_amd import _lib
    lib = _lib.load()
    ptr = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before the device is touched

    def forward(batch=4, seq_len=24, hidden=64, n_answers=3, n_paras=40, dim=128, lens=ptr, cu=None, flags=1, p=0.0):
        return lib.proqa_reader_loss_f16(ptr, lens, cu, batch, seq_len, hidden, ptr, ptr, ptr, ptr, ptr, n_answers, ptr, ptr, 0,
                                         ptr, n_paras, dim, flags, p, 1, 255, 0, ptr, ptr, ptr, ptr, 1 << 30, None)

    def backward(batch=4, seq_len=24, hidden=64, n_answers=3, n_paras=40, dim=128, lens=ptr, cu=None, flags=1, p=0.0):
        return lib.proqa_reader_loss_backward_f16(ptr, lens, cu, batch, seq_len, hidden, ptr, ptr, ptr, ptr, n_answers, ptr, ptr,
                                                  0, ptr, n_paras, dim, flags, p, 1, 255, 0, ptr, ptr, ptr, ptr, ptr, ptr, ptr,
                                                  ptr, 1 << 30, None)
    for call in (forward, backward):
        for bad, word in ((dict(n_paras=3), b"rows"), (dict(dim=64), b"dim=64"), (dict(n_answers=0), b"answer"),
                          (dict(n_answers=1025), b"answer"), (dict(lens=ptr, cu=ptr), b"exactly one"),
                          (dict(lens=None, cu=None), b"exactly one"), (dict(hidden=100), b"hidden=100"),
                          (dict(hidden=2048), b"hidden=2048"), (dict(seq_len=4097), b"seq_len"), (dict(n_paras=65537), b"rows"),
                          (dict(flags=8), b"flags"), (dict(p=1.0), b"p=1")):
            assert call(**bad) == -1, bad
            assert word in lib.proqa_last_error(), (bad, lib.proqa_last_error())
    need = lib.proqa_reader_loss_workspace_bytes(5, 512, 768, 8, 5000)
    assert need % 16 == 0 and need >= 5 * 16 * (2 * 768 + 8) * 4
    assert lib.proqa_reader_loss_workspace_bytes(0, 512, 768, 8, 5000) == 0


def test_reference_error_table_is_reproduced():
    """the GPU test's bounds are four times these numbers; they are measured here, on the CPU"""
    table = G.measure_reference_error()
    assert set(table) == set(G.REFERENCE_ERROR)
    for name, row in table.items():
        for k, v in row.items():
            want = G.REFERENCE_ERROR[name][k]
            assert abs(v - want) <= 0.1 * want + 1e-30, (name, k, v, want)
    l0, l20 = G.train_trajectory()
    assert abs(l0 - G.TRAIN_L0) <= 1e-6 * l0 and abs(l20 - G.TRAIN_L20) <= 1e-6 * l20
    assert l20 < 0.5 * l0
