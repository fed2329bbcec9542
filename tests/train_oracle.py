"""torch restatements of the trainable tower's operators with gradients from torch.autograd -- TEST INFRASTRUCTURE ONLY.

oracle/bert_torch_cpu.py is @torch.no_grad() and frozen, so the arithmetic is restated here (checked against it in
tests/test_train_host.py).  Two modes:

  dtype=float64, storage=None    the reference value: float64 arithmetic on the kernel's own fp16 inputs.
  dtype=float32, storage="fp16"  "the reference's own arithmetic" (apex O1): fp32 arithmetic, and every tensor that
                                 proqa_amd.trainable stores in fp16 is rounded to fp16 at the same point -- in the forward
                                 pass (store()), for the activation gradients (register_hook inside store()) and for the
                                 final gradients of fp16 tensors.  Gradients the module keeps in fp32 (parameter vectors
                                 and embedding tables of the fused operators) are not rounded.

measure(...) helpers return max|a - ref| / max|ref| per tensor, the error measure of the GPU tests.
"""
import math

import torch
import torch.nn.functional as F


def store(x, storage):
    """x as the module stores it: the value rounded to fp16 and, through register_hook, its gradient too."""
    if storage != "fp16":
        return x
    y = x + (x.detach().half().to(x.dtype) - x.detach())
    if y.requires_grad:
        y.register_hook(lambda g: g.half().to(g.dtype))
    return y


def final(g, storage, fp16_tensor):
    """a final gradient as the module keeps it: fp16 for an fp16 tensor, else the compute type"""
    return g.half().to(g.dtype) if storage == "fp16" and fp16_tensor else g


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    scale = ref.abs().max().item()
    return (got - ref).abs().max().item() / scale if scale > 0 else (got - ref).abs().max().item()


def leaf(x, dtype):
    return torch.as_tensor(x).to(dtype).clone().requires_grad_(True)


# ---- operators ------------------------------------------------------------------------------------------------------------

def attention_forward(qkv, qkv_bias, lens, n_heads, storage=None):
    """packed qkv [T, 3H] (before the bias) -> ctx [T, H]; query bias added, key bias dropped, value bias on the output"""
    H = n_heads * 64
    out, row = [], 0
    for n in lens:
        n = int(n)
        blk = qkv[row:row + n]
        q, k, v = blk[:, :H], blk[:, H:2 * H], blk[:, 2 * H:]
        if qkv_bias is not None:
            q = store(q + qkv_bias[:H], storage)
        q, k, v = (t.reshape(n, n_heads, 64).transpose(0, 1) for t in (q, k, v))
        p = torch.softmax(q @ k.transpose(1, 2) * 0.125, -1)
        ctx = store((p @ v).transpose(0, 1).reshape(n, H), storage)
        if qkv_bias is not None:
            ctx = store(ctx + qkv_bias[2 * H:], storage)
        out.append(ctx)
        row += n
    return torch.cat(out, 0)


def attention_backward(qkv, qkv_bias, d_ctx, lens, n_heads, dtype=torch.float64, storage=None):
    x = leaf(qkv, dtype)
    b = None if qkv_bias is None else torch.as_tensor(qkv_bias).to(dtype)
    ctx = attention_forward(x, b, lens, n_heads, storage)
    (g,) = torch.autograd.grad(ctx, x, torch.as_tensor(d_ctx).to(dtype))
    return {"d_qkv": final(g, storage, True)}


def bias_residual_layernorm_forward(x, bias, residual, gamma, beta, eps, storage=None):
    z = x + bias + residual
    return store(F.layer_norm(z, z.shape[-1:], gamma, beta, eps), storage)


def bias_residual_layernorm_backward(dy, x, bias, residual, gamma, eps, dtype=torch.float64, storage=None):
    xs, bs, gs = leaf(x, dtype), leaf(bias, dtype), leaf(gamma, dtype)
    beta = torch.zeros_like(gs).requires_grad_(True)
    y = bias_residual_layernorm_forward(xs, bs, torch.as_tensor(residual).to(dtype), gs, beta, eps, storage)
    dz, dbias, dgamma, dbeta = torch.autograd.grad(y, (xs, bs, gs, beta), torch.as_tensor(dy).to(dtype))
    return {"dz": final(dz, storage, True), "dgamma": dgamma, "dbeta": dbeta, "dbias": dbias}


def gelu(t):
    return 0.5 * t * (1.0 + torch.erf(t * (1.0 / math.sqrt(2.0))))


def bias_gelu_backward(dy, x_pre, bias, dtype=torch.float64, storage=None):
    xs, bs = leaf(x_pre, dtype), leaf(bias, dtype)
    y = store(gelu(xs + bs), storage)
    dx, dbias = torch.autograd.grad(y, (xs, bs), torch.as_tensor(dy).to(dtype))
    return {"dx": final(dx, storage, True), "dbias": dbias}


def embed_layernorm_forward(ids, lens, word, pos, type0, gamma, beta, eps, storage=None):
    rows = [word[ids[b, :int(n)]] + pos[:int(n)] + type0 for b, n in enumerate(lens)]
    z = torch.cat(rows, 0)
    return store(F.layer_norm(z, z.shape[-1:], gamma, beta, eps), storage)


def embed_layernorm_backward(dy, ids, lens, word, pos, type0, gamma, eps, dtype=torch.float64, storage=None):
    w, p, t, g = leaf(word, dtype), leaf(pos, dtype), leaf(type0, dtype), leaf(gamma, dtype)
    beta = torch.zeros_like(g).requires_grad_(True)
    y = embed_layernorm_forward(torch.as_tensor(ids), lens, w, p, t, g, beta, eps, storage)
    d_word, d_pos, d_type0, dgamma, dbeta = torch.autograd.grad(y, (w, p, t, g, beta), torch.as_tensor(dy).to(dtype))
    return {"dgamma": dgamma, "dbeta": dbeta, "d_word": d_word, "d_pos": d_pos, "d_type0": d_type0}


def inbatch_loss(q, c, target=None):
    t = torch.arange(q.shape[0]) if target is None else torch.as_tensor(target).long()
    return F.cross_entropy(q @ c.t(), t)


def inbatch_loss_grad(q, c, target, grad_in=1.0, dtype=torch.float64, storage=None):
    qs, cs = leaf(q, dtype), leaf(c, dtype)
    dq, dc = torch.autograd.grad(inbatch_loss(qs, cs, target) * grad_in, (qs, cs))
    return {"dq": final(dq, storage, True), "dc": final(dc, storage, True)}


def colsum(x, dtype=torch.float64):
    return torch.as_tensor(x).to(dtype).sum(0)


# ---- the tower --------------------------------------------------------------------------------------------------------------

# parameters whose gradient the module receives in fp16 (the weight of a dense product: torch's GEMM backward on the fp16
# cast; the pooler and projection biases, which stay on torch) -- every other gradient leaves a fused operator as fp32
def _grad_is_fp16(key):
    return ("LayerNorm" not in key and "embeddings" not in key and key.endswith(".weight")) or "pooler" in key or key.startswith("proj_")


def tower_forward(sd, input_ids, input_mask, is_query_embed, n_layers, n_heads, eps=1e-12, storage=None):
    """[B, S] ids + right-padded mask -> [B, 128]; sd: key -> tensor of the compute type (leaves for gradients).  The padded
    layout of oracle/bert_torch_cpu.py; with storage="fp16" rounded wherever proqa_amd.trainable holds an fp16 tensor."""
    tower, proj = ("bert_q", "proj_q") if is_query_embed else ("bert_c", "proj_c")

    def P(key):     # the fp16 cast of a master parameter, straight-through; its gradient rounded where the module's is
        x = sd[key]
        if storage != "fp16":
            return x
        y = x + (x.detach().half().to(x.dtype) - x.detach())
        if y.requires_grad and _grad_is_fp16(key):
            y.register_hook(lambda g: g.half().to(g.dtype))
        return y

    st = lambda x: store(x, storage)
    ids = torch.as_tensor(input_ids, dtype=torch.int64)
    mask = torch.as_tensor(input_mask, dtype=torch.bool)
    B, S = ids.shape
    e = tower + ".embeddings."
    x = P(e + "word_embeddings.weight")[ids] + P(e + "token_type_embeddings.weight")[0] + P(e + "position_embeddings.weight")[:S][None]
    H = x.shape[-1]
    h = st(F.layer_norm(x, (H,), P(e + "LayerNorm.weight"), P(e + "LayerNorm.bias"), eps))
    dh = H // n_heads
    add_mask = torch.where(mask, 0.0, torch.finfo(torch.float32).min).to(x.dtype)[:, None, None, :]
    for i in range(n_layers):
        p = f"{tower}.encoder.layer.{i}."

        def heads(name, with_bias):
            y = st(F.linear(h, P(p + f"attention.self.{name}.weight")))
            if with_bias:
                y = st(y + P(p + f"attention.self.{name}.bias"))
            return y.view(B, S, n_heads, dh).transpose(1, 2)

        # the key bias shifts every score of a query alike: dropped, as in the kernels (its gradient is zero)
        q, k, v = heads("query", True), heads("key", False), heads("value", False)
        probs = torch.softmax(q @ k.transpose(-1, -2) * (1.0 / math.sqrt(dh)) + add_mask, dim=-1)
        ctx = st(st((probs @ v).transpose(1, 2).reshape(B, S, H)) + P(p + "attention.self.value.bias"))
        a = st(F.linear(ctx, P(p + "attention.output.dense.weight")))
        h1 = st(F.layer_norm(a + P(p + "attention.output.dense.bias") + h, (H,), P(p + "attention.output.LayerNorm.weight"),
                             P(p + "attention.output.LayerNorm.bias"), eps))
        f = st(gelu(st(F.linear(h1, P(p + "intermediate.dense.weight"))) + P(p + "intermediate.dense.bias")))
        o = st(F.linear(f, P(p + "output.dense.weight")))
        h = st(F.layer_norm(o + P(p + "output.dense.bias") + h1, (H,), P(p + "output.LayerNorm.weight"),
                            P(p + "output.LayerNorm.bias"), eps))
    pooled = st(torch.tanh(st(F.linear(h[:, 0], P(tower + ".pooler.dense.weight"), P(tower + ".pooler.dense.bias")))))
    return st(F.linear(pooled, P(proj + ".weight"), P(proj + ".bias")))


def model_forward(sd, batch, n_layers, n_heads, eps=1e-12, storage=None):
    return {"q": tower_forward(sd, batch["input_ids_q"], batch["input_mask_q"], True, n_layers, n_heads, eps, storage),
            "c": tower_forward(sd, batch["input_ids_c"], batch["input_mask_c"], False, n_layers, n_heads, eps, storage)}


def model_gradients(state_dict, batch, n_layers, n_heads, eps=1e-12, dtype=torch.float64, storage=None, loss_scale=1.0):
    """(loss, {key: gradient of the UNscaled loss}, {'q', 'c'}): one backward of the in-batch loss times loss_scale"""
    sd = {k: leaf(v, dtype) for k, v in state_dict.items()}
    out = model_forward(sd, batch, n_layers, n_heads, eps, storage)
    loss = inbatch_loss(out["q"], out["c"])
    (loss * loss_scale).backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad / loss_scale) for k, v in sd.items()}
    return loss.item(), grads, {k: v.detach() for k, v in out.items()}


# ---- the fixed case of the module tests -----------------------------------------------------------------------------------------

SMALL_CONFIG = dict(vocab_size=120, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512,
                    max_position_embeddings=64, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")


def small_batch(seed=0, pairs=8):
    """8 (question, paragraph) pairs: questions of 3-12 tokens, paragraphs of 5-40, right-padded with id 0"""
    g = torch.Generator().manual_seed(100 + seed)
    lq = torch.randint(3, 13, (pairs,), generator=g)
    lc = torch.randint(5, 41, (pairs,), generator=g)
    idq = torch.randint(1, 120, (pairs, 12), generator=g)
    idc = torch.randint(1, 120, (pairs, 40), generator=g)
    mq = torch.arange(12)[None] < lq[:, None]
    mc = torch.arange(40)[None] < lc[:, None]
    return {"input_ids_q": idq * mq, "input_mask_q": mq, "input_ids_c": idc * mc, "input_mask_c": mc}


def train_steps(state_dict, batch, n_layers, n_heads, steps=20, dtype=torch.float32):
    """`steps` steps of AdamW(lr=1e-3, eps=1e-8, weight_decay=0) with clip_grad_norm_(2.0) on one batch -> [(loss, correct)]
    before every step and after the last"""
    sd = {k: leaf(v, dtype) for k, v in state_dict.items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=1e-3, eps=1e-8, weight_decay=0.0)
    n = batch["input_ids_q"].shape[0]
    trace = []
    for step in range(steps + 1):
        out = model_forward(sd, batch, n_layers, n_heads)
        prod = out["q"] @ out["c"].t()
        loss = F.cross_entropy(prod, torch.arange(n))
        trace.append((loss.item(), int((prod.argmax(-1) == torch.arange(n)).sum())))
        if step == steps:
            break
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(sd.values()), 2.0)
        opt.step()
    return trace
