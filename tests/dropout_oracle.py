"""numpy / torch restatement of the dropout of the trainable towers -- TEST INFRASTRUCTURE ONLY.

The generator and the two mask functions restate proqa_amd/csrc/dropout_rng.h in numpy (Philox4x32-10; a decision is 16
bits of output, kept iff >= thr).  The operators and the tower restate the kernels with the masks as EXPLICIT tensors
D = keep * factor, in the two modes of tests/train_oracle.py (float64 reference; float32 with storage="fp16"), on whose
functions they are built.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import train_oracle as base
from train_oracle import final, leaf, rel_err, store  # noqa: F401  (re-exported for the tests)

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

SITE_EMBEDDINGS = 0


def site_of(layer, which):
    """which: 0 attention probabilities, 1 attention output, 2 FFN output"""
    return 1 + 3 * layer + which


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counter words (arrays or ints, broadcast together), key words (ints) -> four uint32 arrays"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # < 2^64: no wrap
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & np.uint64(MASK32), n2, p0 & np.uint64(MASK32)
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(p):
    return min(65535, int(math.floor(p * 65536 + 0.5)))


def p_eff(p):
    return threshold(p) / 65536.0


def factor(p):
    """the survivors' factor, as the library computes it: fp32 1 / (1 - thr / 65536)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(threshold(p)) / np.float32(65536.0)))


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & MASK32, seed >> 32


def _c3(site, call):
    return (int(site) | (int(call) << 8)) & MASK32


def _decide(words, w, h, p):
    """words: four uint32 arrays; w, h: index arrays of the same shape -> bool keep"""
    word = np.choose(w, words)
    return ((word >> (16 * h).astype(np.uint32)) & np.uint32(0xFFFF)) >= np.uint32(threshold(p))


def hidden_mask(p, seed, site, call, rows, cols, row0=0):
    """bool [rows, cols]: element (row0 + r, c) of a packed [T, cols] matrix is kept"""
    r = (np.arange(rows, dtype=np.int64) + row0)[:, None]
    c = np.arange(cols, dtype=np.int64)[None, :]
    r, c = np.broadcast_arrays(r, c)
    words = philox4x32_10(c >> 3, r, 0, _c3(site, call), *_key(seed))
    return _decide(words, (c & 7) >> 1, c & 1, p)


def probs_mask(p, seed, site, call, pair, n_queries, n_keys=None):
    """bool [n_queries, n_keys]: probability (query i, key j) of (sequence, head) pair = b * n_heads + head is kept"""
    n_keys = n_queries if n_keys is None else n_keys
    i = np.arange(n_queries, dtype=np.int64)[:, None]
    j = np.arange(n_keys, dtype=np.int64)[None, :]
    i, j = np.broadcast_arrays(i, j)
    words = philox4x32_10(j >> 2, i >> 1, pair, _c3(site, call), *_key(seed))
    return _decide(words, j & 3, i & 1, p)


def attention_masks(p, seed, site, call, lens, n_heads):
    """[per sequence: bool tensor [n_heads, n, n]]"""
    return [torch.from_numpy(np.stack([probs_mask(p, seed, site, call, b * n_heads + h, int(n)) for h in range(n_heads)]))
            for b, n in enumerate(lens)]


# ---- operators: D = keep * factor as an explicit tensor of the compute type -------------------------------------------------

def scaled(keep, p, dtype):
    return torch.as_tensor(keep).to(dtype) * factor(p)


def dropout_forward(x, D, storage=None):
    return store(x * D, storage)


def dropout_backward(dy, D, dtype=torch.float64, storage=None):
    return {"dx": final(torch.as_tensor(dy).to(dtype) * D.to(dtype), storage, True)}


def bias_residual_layernorm_dropout_forward(x, bias, residual, gamma, beta, eps, D, storage=None):
    z = (x + bias) * D + residual
    return store(F.layer_norm(z, z.shape[-1:], gamma, beta, eps), storage)


def bias_residual_layernorm_dropout_backward(dy, x, bias, residual, gamma, eps, D, dtype=torch.float64, storage=None):
    xs, bs, gs, rs = leaf(x, dtype), leaf(bias, dtype), leaf(gamma, dtype), leaf(residual, dtype)
    beta = torch.zeros_like(gs).requires_grad_(True)
    y = bias_residual_layernorm_dropout_forward(xs, bs, rs, gs, beta, eps, D.to(dtype), storage)
    dx, dres, dbias, dgamma, dbeta = torch.autograd.grad(y, (xs, rs, bs, gs, beta), torch.as_tensor(dy).to(dtype))
    return {"dx": final(dx, storage, True), "dresidual": final(dres, storage, True), "dgamma": dgamma, "dbeta": dbeta,
            "dbias": dbias}


def attention_dropout_forward(qkv, qkv_bias, lens, n_heads, Ds, storage=None):
    """train_oracle.attention_forward with the probabilities multiplied by Ds[b] [n_heads, n, n]: ctx = (P D) V + b_v
    rowsum(P D) -- the rows of P D do not sum to 1, so the value bias is weighted"""
    H = n_heads * 64
    out, row = [], 0
    for b, n in enumerate(lens):
        n = int(n)
        blk = qkv[row:row + n]
        q, k, v = blk[:, :H], blk[:, H:2 * H], blk[:, 2 * H:]
        if qkv_bias is not None:
            q = store(q + qkv_bias[:H], storage)
        q, k, v = (t.reshape(n, n_heads, 64).transpose(0, 1) for t in (q, k, v))
        a = torch.softmax(q @ k.transpose(1, 2) * 0.125, -1) * Ds[b].to(qkv.dtype)
        ctx = store((a @ v).transpose(0, 1).reshape(n, H), storage)
        if qkv_bias is not None:
            weight = a.sum(-1).transpose(0, 1)[:, :, None]                     # [n, heads, 1]
            ctx = store(ctx + (qkv_bias[2 * H:].reshape(1, n_heads, 64) * weight).reshape(n, H), storage)
        out.append(ctx)
        row += n
    return torch.cat(out, 0)


def attention_dropout_backward(qkv, qkv_bias, d_ctx, lens, n_heads, Ds, dtype=torch.float64, storage=None):
    x = leaf(qkv, dtype)
    b = None if qkv_bias is None else torch.as_tensor(qkv_bias).to(dtype)
    ctx = attention_dropout_forward(x, b, lens, n_heads, Ds, storage)
    (g,) = torch.autograd.grad(ctx, x, torch.as_tensor(d_ctx).to(dtype))
    return {"d_qkv": final(g, storage, True)}


# ---- the tower ----------------------------------------------------------------------------------------------------------------

def tower_masks(p_hidden, p_attn, seed, call, input_mask, hidden, n_layers, n_heads, dtype):
    """The D tensors of one tower pass in the padded layout of train_oracle.tower_forward: {site: [B, S, hidden]} for the
    hidden sites, {site: [B, heads, S, S]} for the probabilities.  Token (b, s) is row cu[b] + s of the packed matrix the
    kernels see; padding positions get 1 (they reach nothing)."""
    mask = torch.as_tensor(input_mask, dtype=torch.bool)
    B, S = mask.shape
    lens = mask.sum(1).clamp(min=1).tolist()
    cu = np.concatenate([[0], np.cumsum(lens)])
    out = {}
    hidden_sites = [SITE_EMBEDDINGS] + [site_of(i, w) for i in range(n_layers) for w in (1, 2)]
    for site in hidden_sites:
        D = torch.ones(B, S, hidden, dtype=dtype)
        if p_hidden > 0:
            keep = hidden_mask(p_hidden, seed, site, call, int(cu[-1]), hidden)
            for b, n in enumerate(lens):
                D[b, :n] = scaled(keep[cu[b]:cu[b] + n], p_hidden, dtype)
        out[site] = D
    for i in range(n_layers):
        site = site_of(i, 0)
        D = torch.ones(B, n_heads, S, S, dtype=dtype)
        if p_attn > 0:
            for b, n in enumerate(lens):
                for h in range(n_heads):
                    D[b, h, :n, :n] = scaled(probs_mask(p_attn, seed, site, call, b * n_heads + h, n), p_attn, dtype)
        out[site] = D
    return out


def tower_forward(sd, input_ids, input_mask, is_query_embed, n_layers, n_heads, masks, eps=1e-12, storage=None):
    """train_oracle.tower_forward with transformers' dropout at the sites of `masks` (tower_masks): after the embedding
    LayerNorm, on the attention probabilities, and on dense + bias before the residual of both LayerNorms."""
    tower, proj = ("bert_q", "proj_q") if is_query_embed else ("bert_c", "proj_c")

    def P(key):
        x = sd[key]
        if storage != "fp16":
            return x
        y = x + (x.detach().half().to(x.dtype) - x.detach())
        if y.requires_grad and base._grad_is_fp16(key):
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
    h = st(h * masks[SITE_EMBEDDINGS])
    dh = H // n_heads
    add_mask = torch.where(mask, 0.0, torch.finfo(torch.float32).min).to(x.dtype)[:, None, None, :]
    for i in range(n_layers):
        p = f"{tower}.encoder.layer.{i}."

        def heads(name, with_bias):
            y = st(F.linear(h, P(p + f"attention.self.{name}.weight")))
            if with_bias:
                y = st(y + P(p + f"attention.self.{name}.bias"))
            return y.view(B, S, n_heads, dh).transpose(1, 2)

        q, k, v = heads("query", True), heads("key", False), heads("value", False)
        probs = torch.softmax(q @ k.transpose(-1, -2) * (1.0 / math.sqrt(dh)) + add_mask, dim=-1) * masks[site_of(i, 0)]
        weight = probs.sum(-1).transpose(1, 2)[..., None]                       # [B, S, heads, 1]
        b_v = (P(p + "attention.self.value.bias").view(1, 1, n_heads, dh) * weight).reshape(B, S, H)
        ctx = st(st((probs @ v).transpose(1, 2).reshape(B, S, H)) + b_v)
        a = st(F.linear(ctx, P(p + "attention.output.dense.weight")))
        h1 = st(F.layer_norm((a + P(p + "attention.output.dense.bias")) * masks[site_of(i, 1)] + h, (H,),
                             P(p + "attention.output.LayerNorm.weight"), P(p + "attention.output.LayerNorm.bias"), eps))
        f = st(base.gelu(st(F.linear(h1, P(p + "intermediate.dense.weight"))) + P(p + "intermediate.dense.bias")))
        o = st(F.linear(f, P(p + "output.dense.weight")))
        h = st(F.layer_norm((o + P(p + "output.dense.bias")) * masks[site_of(i, 2)] + h1, (H,), P(p + "output.LayerNorm.weight"),
                            P(p + "output.LayerNorm.bias"), eps))
    pooled = st(torch.tanh(st(F.linear(h[:, 0], P(tower + ".pooler.dense.weight"), P(tower + ".pooler.dense.bias")))))
    return st(F.linear(pooled, P(proj + ".weight"), P(proj + ".bias")))


def model_forward(sd, batch, n_layers, n_heads, p_hidden, p_attn, seed, call, eps=1e-12, storage=None):
    """both towers as TrainableRetriever.forward runs them: the question tower takes `call`, the paragraph tower call + 1"""
    any_sd = next(iter(sd.values()))
    H = sd["bert_q.embeddings.LayerNorm.weight"].shape[0]
    out = {}
    for side, is_q, c in (("q", True, call), ("c", False, call + 1)):
        masks = tower_masks(p_hidden, p_attn, seed, c & 0xFFFFFF, batch[f"input_mask_{side}"], H, n_layers, n_heads, any_sd.dtype)
        out[side] = tower_forward(sd, batch[f"input_ids_{side}"], batch[f"input_mask_{side}"], is_q, n_layers, n_heads, masks,
                                  eps, storage)
    return out


def model_gradients(state_dict, batch, n_layers, n_heads, p_hidden, p_attn, seed, call, eps=1e-12, dtype=torch.float64,
                    storage=None, loss_scale=1.0):
    """train_oracle.model_gradients with dropout: (loss, {key: gradient of the unscaled loss}, {'q', 'c'})"""
    sd = {k: leaf(v, dtype) for k, v in state_dict.items()}
    out = model_forward(sd, batch, n_layers, n_heads, p_hidden, p_attn, seed, call, eps, storage)
    loss = base.inbatch_loss(out["q"], out["c"])
    (loss * loss_scale).backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad / loss_scale) for k, v in sd.items()}
    return loss.item(), grads, {k: v.detach() for k, v in out.items()}


def train_steps(state_dict, batch, n_layers, n_heads, p_hidden, p_attn, seed, steps=20, dtype=torch.float32):
    """train_oracle.train_steps with dropout in the training passes (step t takes calls 2t, 2t + 1) -> (eval loss, correct)
    after the last step, evaluated without dropout"""
    sd = {k: leaf(v, dtype) for k, v in state_dict.items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=1e-3, eps=1e-8, weight_decay=0.0)
    n = batch["input_ids_q"].shape[0]
    for step in range(steps):
        out = model_forward(sd, batch, n_layers, n_heads, p_hidden, p_attn, seed, 2 * step)
        loss = F.cross_entropy(out["q"] @ out["c"].t(), torch.arange(n))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(sd.values()), 2.0)
        opt.step()
    with torch.no_grad():
        out = base.model_forward(sd, batch, n_layers, n_heads)
        prod = out["q"] @ out["c"].t()
        return F.cross_entropy(prod, torch.arange(n)).item(), int((prod.argmax(-1) == torch.arange(n)).sum())
