"""The tolerance tables of tests/test_trainable_reader_multi_gpu.py, reproduced on the CPU, and what its three questions must
be for the test to mean what it says."""
import pytest
import torch

import reader_train_oracle as oracle


def test_multi_question_tolerance_tables_are_reproduced():
    """Summation order inside torch's CPU kernels may move the figures a little between machines; the GPU test uses the
    recorded figures, this test says when they have drifted."""
    import test_trainable_reader_multi_gpu as G
    forward, worst = G.measure_reference_error()
    print([f"{v:.3e}" for v in forward])
    print("\n".join(f"                  {k:<48} {v:.3e} / {4 * v:.3e}" for k, v in worst.items()))
    assert len(forward) == len(G.FORWARD_REFERENCE_ERROR) == 3
    for got, recorded in zip(forward, G.FORWARD_REFERENCE_ERROR):
        assert got == pytest.approx(recorded, rel=0.25), (got, recorded)
        assert f"{recorded:.3e}" in G.__doc__
    top = max(G.FORWARD_REFERENCE_ERROR)
    assert G.FORWARD_BOUND == 4.0 * top and f"{top:.3e} / {4 * top:.3e}" in G.__doc__
    assert set(worst) == set(G.REFERENCE_ERROR)
    for k, recorded in G.REFERENCE_ERROR.items():
        assert worst[k] == pytest.approx(recorded, rel=0.25), (k, worst[k], recorded)
        assert f"{recorded:.3e}" in G.__doc__ and f"{4 * recorded:.3e}" in G.__doc__, k
        assert G.BOUNDS[k] == 4.0 * recorded
    # every parameter that is compared has a bound; what is left out is zero in float64
    _, _, grads = G.reference()
    for key, g in grads.items():
        if G.zero_by_construction(key) or key.endswith("attention.self.key.bias"):
            assert g.abs().max() == 0, key
        elif key in G.CANCELS:
            sibling, bound_kind = G.CANCELS[key]
            assert g.abs().max() <= 1e-12 * grads[sibling].abs().max() and bound_kind in G.BOUNDS, key
        else:
            assert g.abs().max() > 0 and G.kind(key) in G.BOUNDS, key


def test_the_three_questions_differ_where_the_header_says():
    import test_trainable_reader_multi_gpu as G
    qs = G.questions()
    assert [q["input_ids"].shape for q in qs] == [(5, 40), (2, 33), (1, 40)]
    assert [q["start_positions"].shape[1] for q in qs] == [3, 2, 3] and [q["para_embed"].shape[0] for q in qs] == [40, 25, 7]
    assert [int(q["input_mask_q"][0].sum()) for q in qs] == [6, 5, 6]
    assert not torch.equal(qs[0]["input_ids"][1:3, :33], qs[1]["input_ids"])
    for q in qs:
        lens, po = oracle.para_offsets(q)
        st, en = q["start_positions"], q["end_positions"]
        valid = [(po[b] <= int(s) < lens[b] - 1) and (po[b] <= int(e) < lens[b] - 1)
                 for b in range(len(lens)) for s, e in zip(st[b], en[b])]
        assert any(valid) and q["top5000_labels"].sum() > 0        # every question has a joint and an early term
