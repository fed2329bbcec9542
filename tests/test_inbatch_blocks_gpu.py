"""proqa_inbatch_loss_blocks_f16 / proqa_inbatch_loss_blocks_grad_f16 (the block-diagonal in-batch objective of
pretrain_retriever.py --micro-batches-per-pass) against the single-rectangle calls and tests/inbatch_blocks_oracle.py.

Bits.  A block of at most 512 rows has no column split in proqa_inbatch_eval_f16 (proqa_hip.h), so its lse, gold, dq and dc
must equal the single calls on the block's slices bit for bit -- NaN payloads included: the tensors are compared as
integers.  The per-block loss is a fixed-order fp32 sum of our own and torch's .mean() in inbatch_loss is another order of
the same numbers, so the loss is held to the float64 mean of the (bit-equal) lse - gold within n * 2^-23 * max|lse - gold|
(n fp32 additions), and to the oracle within 1e-3 absolute, the figure of tests/test_inbatch_gpu.py.  The block of 600 rows
is past the split threshold: it is held to the oracle only.

Accuracy.  Error measure per tensor: max|gpu - ref| / max|ref| (train_oracle.rel_err) against the float64 oracle; bound:
four times the same measure of the oracle's storage="fp16" mode, the maximum over the cases -- the rule of
tests/test_train_ops_gpu.py.  measure_reference_error() below, run on the CPU (tests/test_pretrain_passes_host.py keeps
the table current), grad_in = GRAD_IN cycled over the blocks:

    output   measured    bound
    dq       4.007e-04   1.603e-03
    dc       3.695e-04   1.478e-03

The [1] case has a zero gradient (one row is its own gold): there the error is taken relative to max|c| (dq) and max|q|
(dc), the size of the terms that cancel, as in tests/test_train_ops_gpu.py.
"""
import functools

import pytest
import torch

import inbatch_blocks_oracle as oracle

pytestmark = pytest.mark.gpu

# block starts off the multiples of 32, tiles that straddle a block's end, one-row blocks, several tiles per block
CASES = {"1": [1], "32": [32], "33": [33], "80x3": [80, 80, 80], "ragged": [31, 1, 33, 80, 32], "6x3": [6, 6, 6],
         "600+40": [600, 40]}
BIT_CASES = [k for k, v in CASES.items() if max(v) <= 512]
GRAD_IN = (1.0, 1024.0, 0.125)
REFERENCE_ERROR = {"dq": 4.007e-04, "dc": 3.695e-04}
BOUNDS = {k: 4.0 * v for k, v in REFERENCE_ERROR.items()}
LOSS_TOLERANCE = 1e-3


def grad_in_of(sizes):
    return [GRAD_IN[m % len(GRAD_IN)] for m in range(len(sizes))]


@functools.lru_cache(maxsize=None)
def case(name):
    """(q, c fp16 CPU tensors, block sizes, float64 oracle with grad_in_of) -- computed once, never modified"""
    sizes = CASES[name]
    n = sum(sizes)
    g = torch.Generator().manual_seed(1000 + n)
    q = (0.3 * torch.randn(n, 128, generator=g)).half()
    c = (0.3 * torch.randn(n, 128, generator=g)).half()
    return q, c, sizes, oracle.evaluate(q, c, sizes, grad_in_of(sizes))


def gradient_error(got, ref, q, c):
    """{'dq', 'dc'}: rel_err, or for an all-zero reference gradient the error relative to the terms that cancel"""
    err = {}
    for k, other in (("dq", c), ("dc", q)):
        if float(ref[k].abs().max()) == 0.0:
            err[k] = float((got[k].double() - ref[k]).abs().max()) / float(other.double().abs().max())
        else:
            err[k] = oracle.rel_err(got[k], ref[k])
    return err


def measure_reference_error():
    """{'dq', 'dc'}: max over CASES of the storage="fp16" oracle's error against float64 -- CPU only"""
    worst = {"dq": 0.0, "dc": 0.0}
    for name in CASES:
        q, c, sizes, ref = case(name)
        got = oracle.evaluate(q, c, sizes, grad_in_of(sizes), dtype=torch.float32, storage="fp16")
        for k, v in gradient_error(got, ref, q, c).items():
            worst[k] = max(worst[k], v)
    return worst


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def run_blocks(q, c, sizes, grad_in, dev):
    """the two block calls -> {'lse', 'gold', 'loss', 'dq', 'dc'} on the device"""
    from proqa_amd.inbatch import block_offsets, inbatch_eval_blocks
    from proqa_amd.trainable import inbatch_loss_blocks_grad
    q, c = q.to(dev), c.to(dev)
    offsets = block_offsets(sizes, q.shape[0])
    out = inbatch_eval_blocks(q, c, offsets)
    g = torch.tensor(grad_in, dtype=torch.float32, device=dev)
    out["dq"], out["dc"] = inbatch_loss_blocks_grad(q, c, offsets, out["lse"], g)
    return out


def run_single(q, c, grad_in, dev):
    """the single-rectangle calls on one block's slices"""
    from proqa_amd.inbatch import inbatch_eval
    from proqa_amd.trainable import inbatch_loss_grad
    q, c = q.to(dev).contiguous(), c.to(dev).contiguous()
    ev = inbatch_eval(q, c)
    dq, dc = inbatch_loss_grad(q, c, None, ev["lse"], torch.tensor(grad_in, dtype=torch.float32, device=dev))
    return {"lse": ev["lse"], "gold": ev["gold"], "dq": dq, "dc": dc}


def assert_block_equals_single(out, q, c, sizes, grad_in, dev, blocks=None):
    o = oracle.offsets_of(sizes)
    for m in (range(len(sizes)) if blocks is None else blocks):
        single = run_single(q[o[m]:o[m + 1]], c[o[m]:o[m + 1]], grad_in[m], dev)
        for k, want in single.items():
            assert torch.equal(bits(out[k][o[m]:o[m + 1]]), bits(want)), (sizes, m, k)
        # the loss: a fixed-order fp32 mean of the same lse - gold
        diff = (single["lse"].double() - single["gold"].double()).cpu()
        if bool(torch.isfinite(diff).all()):
            slack = sizes[m] * 2.0 ** -23 * float(diff.abs().max()) + 1e-45
            assert abs(float(out["loss"][m]) - float(diff.mean())) <= slack, (sizes, m)


@pytest.mark.parametrize("name", BIT_CASES)
def test_every_block_has_the_bits_of_the_single_calls(gpu_device, name):
    q, c, sizes, _ = case(name)
    grad_in = grad_in_of(sizes)
    out = run_blocks(q, c, sizes, grad_in, gpu_device)
    assert_block_equals_single(out, q, c, sizes, grad_in, gpu_device)
    again = run_blocks(q, c, sizes, grad_in, gpu_device)
    for k in out:            # no atomics: the same bits every run
        assert torch.equal(bits(out[k]), bits(again[k])), k


@pytest.mark.parametrize("name", ["1", "33", "80x3"])
def test_one_block_is_inbatch_loss(gpu_device, name):
    """M = 1 over all rows: the bits of inbatch_eval / inbatch_loss_grad on the whole rectangle, and through autograd the
    gradients of inbatch_loss"""
    from proqa_amd.trainable import inbatch_loss, inbatch_loss_blocks
    q, c, sizes, _ = case(name)
    n = sum(sizes)
    out = run_blocks(q, c, [n], [0.125], gpu_device)
    assert_block_equals_single(out, q, c, [n], [0.125], gpu_device)
    grads = []
    for fn in (lambda a, b: inbatch_loss(a, b), lambda a, b: inbatch_loss_blocks(a, b, [n]).sum()):
        a, b = q.to(gpu_device).requires_grad_(True), c.to(gpu_device).requires_grad_(True)
        loss = fn(a, b)
        (loss * 8.0).backward()
        grads.append((loss.detach(), a.grad, b.grad))
    assert torch.equal(bits(grads[0][1]), bits(grads[1][1])) and torch.equal(bits(grads[0][2]), bits(grads[1][2]))
    assert abs(float(grads[0][0]) - float(grads[1][0])) <= n * 2.0 ** -23 * 16.0


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_float64_oracle(gpu_device, name):
    q, c, sizes, ref = case(name)
    out = {k: v.cpu() for k, v in run_blocks(q, c, sizes, grad_in_of(sizes), gpu_device).items()}
    err = gradient_error(out, ref, q, c)
    loss_err = float((out["loss"].double() - ref["loss"]).abs().max())
    stat_err = max(float((out[k].double() - ref[k]).abs().max()) for k in ("lse", "gold"))
    print(f"{name}: dq {err['dq']:.3e} (bound {BOUNDS['dq']:.3e}) dc {err['dc']:.3e} (bound {BOUNDS['dc']:.3e}) "
          f"loss {loss_err:.3e} lse/gold {stat_err:.3e} (bound {LOSS_TOLERANCE:.0e})")
    assert err["dq"] <= BOUNDS["dq"] and err["dc"] <= BOUNDS["dc"]
    assert loss_err <= LOSS_TOLERANCE and stat_err <= LOSS_TOLERANCE


def test_the_gradient_is_linear_in_grad_in_per_block(gpu_device):
    """a power of two scales the fp32 gradient exactly, so the fp16 results scale exactly wherever both are normal numbers
    (|x| >= 2^-14, taken with a factor 2 of margin); below that the two roundings may differ by one subnormal step, 2^-24"""
    q, c, sizes, _ = case("ragged")
    o = oracle.offsets_of(sizes)
    ones = run_blocks(q, c, sizes, [1.0] * len(sizes), gpu_device)
    mixed = run_blocks(q, c, sizes, grad_in_of(sizes), gpu_device)
    for m, g in enumerate(grad_in_of(sizes)):
        for k in ("dq", "dc"):
            base, got = ones[k][o[m]:o[m + 1]].float(), mixed[k][o[m]:o[m + 1]].float()
            want = base * g
            normal = (base.abs() >= 2.0 ** -13) & (want.abs() >= 2.0 ** -13)
            assert torch.equal(got[normal], want[normal]), (m, k)
            assert float((got - want).abs().max()) <= max(g, 1.0) * 2.0 ** -24, (m, k)     # (a subnormal base, scaled up)
    assert torch.equal(bits(ones["loss"]), bits(mixed["loss"]))


def test_an_infinite_grad_in_reaches_its_own_block_only(gpu_device):
    q, c, sizes, _ = case("ragged")
    o = oracle.offsets_of(sizes)
    grad_in = grad_in_of(sizes)
    clean = run_blocks(q, c, sizes, grad_in, gpu_device)
    victim = 2
    hit = run_blocks(q, c, sizes, grad_in[:victim] + [float("inf")] + grad_in[victim + 1:], gpu_device)
    for k in ("dq", "dc"):
        inside = hit[k][o[victim]:o[victim + 1]]
        assert not bool(torch.isfinite(inside).any()), k
        keep = torch.ones(sum(sizes), dtype=torch.bool, device=gpu_device)
        keep[o[victim]:o[victim + 1]] = False
        assert torch.equal(bits(hit[k])[keep], bits(clean[k])[keep]), k


@pytest.mark.parametrize("poison", [60000.0, -60000.0, float("inf"), float("nan")])
def test_a_poisoned_block_stays_inside_itself(gpu_device, poison):
    """rows of ONE block replaced in q and c: every other block keeps its bits, and the poisoned block is what the single
    calls make of those rows"""
    q, c, sizes, _ = case("ragged")
    o = oracle.offsets_of(sizes)
    grad_in = grad_in_of(sizes)
    clean = run_blocks(q, c, sizes, grad_in, gpu_device)
    for victim in (0, 3):
        pq, pc = q.clone(), c.clone()
        pq[o[victim]:o[victim + 1]:2] = poison
        pc[o[victim] + 1:o[victim + 1]:3] = -poison
        pc[o[victim + 1] - 1] = poison                     # the row next to the following block's first
        hit = run_blocks(pq, pc, sizes, grad_in, gpu_device)
        keep = torch.ones(sum(sizes), dtype=torch.bool, device=gpu_device)
        keep[o[victim]:o[victim + 1]] = False
        for k in ("lse", "gold", "dq", "dc"):
            assert torch.equal(bits(hit[k])[keep], bits(clean[k])[keep]), (victim, k)
        others = [m for m in range(len(sizes)) if m != victim]
        assert torch.equal(bits(hit["loss"])[others], bits(clean["loss"])[others])
        assert_block_equals_single(hit, pq, pc, sizes, grad_in, gpu_device, blocks=[victim])


def test_autograd_node(gpu_device):
    """inbatch_loss_blocks: fp32 [M] with gradients; (losses / G).sum().backward() is the closed form with grad_in = 1 / G"""
    from proqa_amd.trainable import inbatch_loss_blocks
    q, c, sizes, _ = case("80x3")
    G = 4
    a, b = q.to(gpu_device).requires_grad_(True), c.to(gpu_device).requires_grad_(True)
    losses = inbatch_loss_blocks(a, b, sizes)
    assert losses.shape == (3,) and losses.dtype == torch.float32 and losses.requires_grad
    (losses / G).sum().backward()
    want = run_blocks(q, c, sizes, [1.0 / G] * 3, gpu_device)
    assert torch.equal(bits(a.grad), bits(want["dq"])) and torch.equal(bits(b.grad), bits(want["dc"]))
    assert torch.equal(bits(losses.detach()), bits(want["loss"]))
    with pytest.raises(ValueError, match="sum to"):
        inbatch_loss_blocks(a, b, [80, 80])
    with pytest.raises(ValueError, match="positive"):
        inbatch_loss_blocks(a, b, [240, 0])
