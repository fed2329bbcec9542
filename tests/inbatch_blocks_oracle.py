"""Float64 oracle of the block-diagonal in-batch objective (proqa_inbatch_loss_blocks_f16 and its gradient) -- TEST
INFRASTRUCTURE ONLY.

Block m owns the next block_sizes[m] rows of BOTH q and c; its loss is CrossEntropyLoss(q_m @ c_m.T, arange), and the
objective that is differentiated is sum_m grad_in[m] * loss_m.  Two routes to the gradient: torch.autograd (evaluate), and
the closed form the kernels use (closed_form), d s[i, j] = grad_in[m] / n_m (softmax(s)[i, j] - [i == j]) inside block m.
The modes are tests/train_oracle.py's: dtype=float64 / storage=None is the reference value on the kernel's own fp16
inputs; dtype=float32 / storage="fp16" is the reference's own arithmetic, the final gradients rounded to fp16.
"""
import torch
import torch.nn.functional as F

from train_oracle import final, leaf, rel_err  # noqa: F401  (rel_err: the GPU tests' error measure)


def offsets_of(block_sizes):
    o = [0]
    for b in block_sizes:
        o.append(o[-1] + int(b))
    return o


def evaluate(q, c, block_sizes, grad_in=None, dtype=torch.float64, storage=None):
    """-> {'loss': [M], 'lse': [n], 'gold': [n], 'dq': [n, 128], 'dc': [n, 128]}; grad_in: M numbers (default: ones)"""
    o = offsets_of(block_sizes)
    assert o[-1] == q.shape[0] == c.shape[0] and all(b >= 1 for b in block_sizes)
    g = torch.ones(len(block_sizes), dtype=dtype) if grad_in is None else torch.as_tensor(grad_in, dtype=dtype)
    qs, cs = leaf(q, dtype), leaf(c, dtype)
    losses, lse, gold = [], [], []
    for m in range(len(block_sizes)):
        s = qs[o[m]:o[m + 1]] @ cs[o[m]:o[m + 1]].t()
        losses.append(F.cross_entropy(s, torch.arange(s.shape[0])))
        lse.append(torch.logsumexp(s.detach(), -1))
        gold.append(s.detach().diagonal())
    losses = torch.stack(losses)
    dq, dc = torch.autograd.grad((losses * g).sum(), (qs, cs))
    return {"loss": losses.detach(), "lse": torch.cat(lse), "gold": torch.cat(gold), "dq": final(dq, storage, True),
            "dc": final(dc, storage, True)}


def closed_form(q, c, block_sizes, grad_in=None, dtype=torch.float64):
    """the kernels' formula, without autograd -> {'loss', 'dq', 'dc'}"""
    o = offsets_of(block_sizes)
    g = torch.ones(len(block_sizes), dtype=dtype) if grad_in is None else torch.as_tensor(grad_in, dtype=dtype)
    q, c = torch.as_tensor(q).to(dtype), torch.as_tensor(c).to(dtype)
    dq, dc, losses = torch.zeros_like(q), torch.zeros_like(c), []
    for m in range(len(block_sizes)):
        qm, cm = q[o[m]:o[m + 1]], c[o[m]:o[m + 1]]
        s = qm @ cm.t()
        lse = torch.logsumexp(s, -1)
        losses.append((lse - s.diagonal()).mean())
        ds = g[m] / s.shape[0] * (torch.exp(s - lse[:, None]) - torch.eye(s.shape[0], dtype=dtype))
        dq[o[m]:o[m + 1]] = ds @ cm
        dc[o[m]:o[m + 1]] = ds.t() @ qm
    return {"loss": torch.stack(losses), "dq": dq, "dc": dc}
