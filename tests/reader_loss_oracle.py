"""Float64 restatement of the reader's training objective (proqa_reader_loss_f16 / _backward_f16 in proqa_hip.h;
qa/bert_retrieve_qa.py:64-171 of the reference with --shared-norm or without, joint loss, early loss).

`forward` is differentiable torch code (autograd checks the closed forms of `evaluate` against it); `evaluate` returns the
loss and the closed-form gradients.  storage="fp16" is the reference's own arithmetic under apex O1: the logits are rounded
to fp16, d_hidden and d_q are rounded to fp16, everything else is float32.  storage="f64" rounds nothing.

Operands: hidden [B, L, H] (padded; rows at or past lens[b] are ignored), lens and para_offset (lists), qa_w [2, H],
qa_b [2], q [128], para [P, 128], labels [P], start / end [B, A] (-1 = padding), keep (optional bool [B, L, H], the dropout
mask of the head) and factor (the survivors' scale).
"""
import torch


def _mask(L, lens, para_offset):
    m = torch.zeros((len(lens), L), dtype=torch.bool)
    for b, (n, p0) in enumerate(zip(lens, para_offset)):
        m[b, max(p0, 0):max(n - 1, 0)] = True
    return m


def _valid_pairs(mask, start, end):
    B, A = start.shape
    out = []
    for b in range(B):
        for a in range(A):
            s, e = int(start[b, a]), int(end[b, a])
            if 0 <= s < mask.shape[1] and 0 <= e < mask.shape[1] and mask[b, s] and mask[b, e]:
                out.append((b, a, s, e))
    return out


def _dropped(hidden, keep, factor, dtype):
    x = hidden.to(dtype)
    if keep is not None:
        x = x * keep.to(dtype) * torch.tensor(factor, dtype=torch.float32).to(dtype)
    return x


def forward(hidden, qa_w, qa_b, q, para, labels, start, end, lens, para_offset, shared_norm=True, early=True, keep=None,
            factor=1.0, storage="f64"):
    """-> dict(loss, joint, early, logits [B, L, 2] unmasked, plus the intermediates `evaluate` needs)"""
    dtype = torch.float64 if storage == "f64" else torch.float32
    B, L, _ = hidden.shape
    x = _dropped(hidden, keep, factor, dtype)
    logits = x @ qa_w.to(dtype).t() + qa_b.to(dtype)
    if storage == "fp16":
        logits = logits.half().to(dtype)
    mask = _mask(L, lens, para_offset)
    s, e = logits[..., 0], logits[..., 1]
    neg = torch.tensor(float("-inf"), dtype=dtype)
    if shared_norm:
        zs = torch.logsumexp(s[mask], 0).expand(B) if mask.any() else neg.expand(B)
        ze = torch.logsumexp(e[mask], 0).expand(B) if mask.any() else neg.expand(B)
    else:
        zs = torch.stack([torch.logsumexp(s[b][mask[b]], 0) if mask[b].any() else neg for b in range(B)])
        ze = torch.stack([torch.logsumexp(e[b][mask[b]], 0) if mask[b].any() else neg for b in range(B)])
    scores = para.to(dtype) @ q.to(dtype)
    log_r = scores - torch.logsumexp(scores, 0)
    pairs = _valid_pairs(mask, start, end)
    zero = torch.zeros((), dtype=dtype)
    if pairs:
        l = torch.stack([s[b, i] - zs[b] + e[b, j] - ze[b] + log_r[b] for b, _, i, j in pairs])
        joint = -torch.logsumexp(l, 0)
    else:
        l, joint = None, zero
    gold = labels != 0
    early_on = bool(early) and bool(gold.any())
    early_loss = -torch.logsumexp(log_r[gold], 0) if early_on else zero
    return dict(loss=joint + early_loss, joint=joint, early=early_loss, logits=logits, x=x, mask=mask, zs=zs, ze=ze,
                log_r=log_r, pairs=pairs, l=l, gold=gold, early_on=early_on)


def evaluate(hidden, qa_w, qa_b, q, para, labels, start, end, lens, para_offset, shared_norm=True, early=True, keep=None,
             factor=1.0, storage="f64", grad=1.0):
    """The loss and its closed-form gradients times `grad` -> dict(loss, joint, early, logits, d_hidden, d_qa_w, d_qa_b, d_q)"""
    with torch.no_grad():
        f = forward(hidden, qa_w, qa_b, q, para, labels, start, end, lens, para_offset, shared_norm, early, keep, factor,
                    storage)
        dtype = f["logits"].dtype
        B, L, H = hidden.shape
        mask, s, e = f["mask"], f["logits"][..., 0], f["logits"][..., 1]
        ds, de = torch.zeros((B, L), dtype=dtype), torch.zeros((B, L), dtype=dtype)
        omega = torch.zeros(B, dtype=dtype)
        if f["pairs"]:
            w = torch.exp(f["l"] + f["joint"])
            for (b, _, i, j), v in zip(f["pairs"], w):
                omega[b] += v
                ds[b, i] -= v
                de[b, j] -= v
            c = torch.ones(B, dtype=dtype) if shared_norm else omega
            for b in range(B):
                m = mask[b]
                if m.any():
                    ds[b][m] += c[b] * torch.exp(s[b][m] - f["zs"][b])
                    de[b][m] += c[b] * torch.exp(e[b][m] - f["ze"][b])
        r = torch.exp(f["log_r"])
        drank = torch.zeros_like(r)
        if f["pairs"]:
            drank += r
            drank[:B] -= omega
        if f["early_on"]:
            g = torch.zeros_like(r)
            g[f["gold"]] = r[f["gold"]] / r[f["gold"]].sum()
            drank += r - g
        gr = torch.tensor(grad, dtype=dtype)
        dlogit = gr * torch.stack([ds, de], -1)                       # [B, L, 2]
        d_hidden = dlogit @ qa_w.to(dtype)
        if keep is not None:
            d_hidden = d_hidden * keep.to(dtype) * torch.tensor(factor, dtype=torch.float32).to(dtype)
        d_qa_w = torch.einsum("blk,blh->kh", dlogit, f["x"])
        d_qa_b = dlogit.sum((0, 1))
        d_q = (gr * drank) @ para.to(dtype)
        if storage == "fp16":
            d_hidden, d_q = d_hidden.half().to(dtype), d_q.half().to(dtype)
        return dict(loss=f["loss"], joint=f["joint"], early=f["early"], logits=f["logits"], d_hidden=d_hidden, d_qa_w=d_qa_w,
                    d_qa_b=d_qa_b, d_q=d_q)


def autograd(hidden, qa_w, qa_b, q, para, labels, start, end, lens, para_offset, shared_norm=True, early=True, keep=None,
             factor=1.0):
    """The same gradients from torch.autograd on `forward` in float64."""
    leaves = [t.double().clone().requires_grad_(True) for t in (hidden, qa_w, qa_b, q)]
    f = forward(*leaves, para, labels, start, end, lens, para_offset, shared_norm, early, keep, factor)
    if not f["loss"].requires_grad:      # no valid pair and no gold label: the loss is the constant 0
        return dict(loss=f["loss"].detach(), d_hidden=torch.zeros_like(leaves[0]), d_qa_w=torch.zeros_like(leaves[1]),
                    d_qa_b=torch.zeros_like(leaves[2]), d_q=torch.zeros_like(leaves[3]))
    grads = torch.autograd.grad(f["loss"], leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    return dict(loss=f["loss"].detach(), d_hidden=grads[0], d_qa_w=grads[1], d_qa_b=grads[2], d_q=grads[3])


OUTPUTS = ("loss", "logits", "d_hidden", "d_qa_w", "d_qa_b", "d_q")


def error(got, ref, floor=0.0):
    """max|got - ref| / max(max|ref|, floor): the measure of the GPU test's bounds"""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    got = torch.as_tensor(got).to(torch.float64)
    scale = max(float(ref.abs().max()) if ref.numel() else 0.0, floor)
    diff = float((got - ref).abs().max()) if ref.numel() else 0.0
    return diff / scale if scale > 0 else diff
