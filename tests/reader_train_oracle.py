"""torch restatements of the typed embedding operator and of the trainable reader -- TEST INFRASTRUCTURE ONLY.

The modes are train_oracle's: dtype=float64 / storage=None is the reference value, dtype=float32 / storage="fp16" is "the
reference's own arithmetic" (fp32 sums, fp16 wherever proqa_amd stores fp16).  The reader model is the typed tower (the
layers of train_oracle.tower_forward, the embeddings with segment ids, the last hidden state instead of the pooler), the
question tower of train_oracle on row 0 of input_ids_q, and reader_loss_oracle.forward on the padded hidden states.
"""
import math

import torch
import torch.nn.functional as F

import reader_loss_oracle as RL
import train_oracle as T
from train_oracle import SMALL_CONFIG, final, leaf, rel_err, store  # noqa: F401  (re-exported for the tests)


# ---- the typed embedding operator -----------------------------------------------------------------------------------------

def _rows(ids, type_ids, lens, vocab, n_types):
    """per sequence: (word rows, type rows) as the kernels read them -- an id outside its table reads row 0"""
    out = []
    for b, n in enumerate(lens):
        n = int(n)
        i = torch.as_tensor(ids)[b, :n].long()
        t = torch.zeros(n, dtype=torch.int64) if type_ids is None else torch.as_tensor(type_ids)[b, :n].long()
        i = torch.where((i < 0) | (i >= vocab), torch.zeros_like(i), i)
        t = torch.where((t < 0) | (t >= n_types), torch.zeros_like(t), t)
        out.append((i, t))
    return out


def embed_typed_forward(ids, type_ids, lens, word, pos, types, gamma, beta, eps, storage=None):
    rows = [word[i] + pos[:len(i)] + types[t] for i, t in _rows(ids, type_ids, lens, word.shape[0], types.shape[0])]
    z = torch.cat(rows, 0)
    return store(F.layer_norm(z, z.shape[-1:], gamma, beta, eps), storage)


def embed_typed_backward_autograd(dy, ids, type_ids, lens, word, pos, types, gamma, eps, dtype=torch.float64, storage=None):
    w, p, t, g = leaf(word, dtype), leaf(pos, dtype), leaf(types, dtype), leaf(gamma, dtype)
    beta = torch.zeros_like(g).requires_grad_(True)
    y = embed_typed_forward(ids, type_ids, lens, w, p, t, g, beta, eps, storage)
    d_word, d_pos, d_types, dgamma, dbeta = torch.autograd.grad(y, (w, p, t, g, beta), torch.as_tensor(dy).to(dtype))
    return {"dgamma": dgamma, "dbeta": dbeta, "d_word": d_word, "d_pos": d_pos, "d_types": d_types}


def embed_typed_backward(dy, ids, type_ids, lens, word, pos, types, gamma, eps, dtype=torch.float64, storage=None):
    """The closed form the kernel evaluates: dz = rstd (a - mean(a) - xhat mean(a xhat)), a = dy gamma, scattered to the
    three tables.  Every output is a parameter gradient, kept in the compute type: storage="fp16" rounds nothing here (dy
    and the tables are fp16 already), the mode is fp32 arithmetic."""
    word, pos, types, gamma = (torch.as_tensor(x).to(dtype) for x in (word, pos, types, gamma))
    dy = torch.as_tensor(dy).to(dtype)
    out = {"dgamma": torch.zeros_like(gamma), "dbeta": torch.zeros_like(gamma), "d_word": torch.zeros_like(word),
           "d_pos": torch.zeros_like(pos), "d_types": torch.zeros_like(types)}
    row = 0
    for i, t in _rows(ids, type_ids, lens, word.shape[0], types.shape[0]):
        n = len(i)
        z = word[i] + pos[:n] + types[t]
        g = dy[row:row + n]
        mean = z.mean(-1, keepdim=True)
        rstd = torch.rsqrt(((z - mean) ** 2).mean(-1, keepdim=True) + eps)
        xhat = (z - mean) * rstd
        a = g * gamma
        dz = rstd * (a - a.mean(-1, keepdim=True) - xhat * (a * xhat).mean(-1, keepdim=True))
        out["dgamma"] += (g * xhat).sum(0)
        out["dbeta"] += g.sum(0)
        out["d_word"].index_add_(0, i, dz)
        out["d_pos"][:n] += dz
        out["d_types"].index_add_(0, t, dz)
        row += n
    return out


# ---- the reader -----------------------------------------------------------------------------------------------------------

def _cast(sd, key, storage):
    """the fp16 cast of a master, straight-through; its gradient rounded where the module's is (train_oracle's rule)"""
    x = sd[key]
    if storage != "fp16":
        return x
    y = x + (x.detach().half().to(x.dtype) - x.detach())
    if y.requires_grad and T._grad_is_fp16(key):
        y.register_hook(lambda g: g.half().to(g.dtype))
    return y


def typed_tower_hidden(sd, tower, input_ids, segment_ids, input_mask, n_layers, n_heads, eps=1e-12, storage=None):
    """[B, S] ids, segment ids, right-padded mask -> the last hidden state [B, S, H] (padded); the layers of
    train_oracle.tower_forward"""
    P = lambda key: _cast(sd, key, storage)
    st = lambda x: store(x, storage)
    ids = torch.as_tensor(input_ids, dtype=torch.int64)
    seg = torch.as_tensor(segment_ids, dtype=torch.int64)
    mask = torch.as_tensor(input_mask, dtype=torch.bool)
    B, S = ids.shape
    e = tower + ".embeddings."
    x = P(e + "word_embeddings.weight")[ids] + P(e + "token_type_embeddings.weight")[seg] + P(e + "position_embeddings.weight")[:S][None]
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

        q, k, v = heads("query", True), heads("key", False), heads("value", False)
        probs = torch.softmax(q @ k.transpose(-1, -2) * (1.0 / math.sqrt(dh)) + add_mask, dim=-1)
        ctx = st(st((probs @ v).transpose(1, 2).reshape(B, S, H)) + P(p + "attention.self.value.bias"))
        a = st(F.linear(ctx, P(p + "attention.output.dense.weight")))
        h1 = st(F.layer_norm(a + P(p + "attention.output.dense.bias") + h, (H,), P(p + "attention.output.LayerNorm.weight"),
                             P(p + "attention.output.LayerNorm.bias"), eps))
        f = st(T.gelu(st(F.linear(h1, P(p + "intermediate.dense.weight"))) + P(p + "intermediate.dense.bias")))
        o = st(F.linear(f, P(p + "output.dense.weight")))
        h = st(F.layer_norm(o + P(p + "output.dense.bias") + h1, (H,), P(p + "output.LayerNorm.weight"),
                            P(p + "output.LayerNorm.bias"), eps))
    return h


def para_offsets(batch):
    """(lens, para_offset) as lists: the first True of paragraph_mask, or the length"""
    lens = [int(n) for n in torch.as_tensor(batch["input_mask"]).bool().sum(1)]
    pm = torch.as_tensor(batch["paragraph_mask"]).bool()
    return lens, [int(pm[b].int().argmax()) if pm[b].any() else lens[b] for b in range(len(lens))]


def model_forward(sd, batch, n_layers, n_heads, shared_norm=True, early=True, eps=1e-12, storage=None):
    """sd: BertRetrieveQA's keys -> tensors of the compute type.  -> reader_loss_oracle.forward's dict plus hidden and q"""
    hidden = typed_tower_hidden(sd, "bert", batch["input_ids"], batch["segment_ids"], batch["input_mask"], n_layers, n_heads,
                                eps, storage)
    retr = {k[len("retriever."):]: v for k, v in sd.items() if k.startswith("retriever.")}
    q = T.tower_forward(retr, batch["input_ids_q"][:1], batch["input_mask_q"][:1], True, n_layers, n_heads, eps, storage)[0]
    lens, po = para_offsets(batch)
    para = torch.as_tensor(batch["para_embed"])
    f = RL.forward(hidden, sd["qa_outputs.weight"], sd["qa_outputs.bias"], q, para, torch.as_tensor(batch["top5000_labels"]).reshape(-1),
                   torch.as_tensor(batch["start_positions"]), torch.as_tensor(batch["end_positions"]), lens, po, shared_norm, early,
                   storage="fp16" if storage == "fp16" else "f64")
    return dict(f, hidden=hidden, q=q)


def model_gradients(state_dict, batch, n_layers, n_heads, shared_norm=True, early=True, eps=1e-12, dtype=torch.float64,
                    storage=None, loss_scale=1.0):
    """({'loss', 'joint', 'early'} floats, {key: gradient of the UNscaled loss}, forward dict)"""
    sd = {k: leaf(v, dtype) for k, v in state_dict.items()}
    f = model_forward(sd, batch, n_layers, n_heads, shared_norm, early, eps, storage)
    (f["loss"] * loss_scale).backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad / loss_scale) for k, v in sd.items()}
    return {k: f[k].item() for k in ("loss", "joint", "early")}, grads, f


def train_steps(state_dict, batch, n_layers, n_heads, steps=20, dtype=torch.float32, lr=1e-3, max_grad_norm=2.0):
    """`steps` steps of AdamW(lr, eps=1e-8, weight_decay=0) with clip_grad_norm_ on one batch -> the losses before every
    step and after the last"""
    sd = {k: leaf(v, dtype) for k, v in state_dict.items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=lr, eps=1e-8, weight_decay=0.0)
    trace = []
    for step in range(steps + 1):
        loss = model_forward(sd, batch, n_layers, n_heads)["loss"]
        trace.append(loss.item())
        if step == steps:
            break
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for p in sd.values() if p.grad is not None], max_grad_norm)
        opt.step()
    return trace


# ---- the fixed case of the module tests -----------------------------------------------------------------------------------

READER_LENS = (40, 33, 21, 9, 7)
QUESTION_PART = 6          # [CLS] q [SEP]: segment 0; the paragraph and the final [SEP]: segment 1
N_PARAS, N_ANSWERS = 40, 3


def small_reader_batch(seed=0):
    """SMALL_CONFIG's batch: 5 sequences of 40 / 33 / 21 / 9 / 7 tokens, the last with an empty paragraph; the answers and
    gold labels of tests/golden/make_reader_loss_golden.py's `both` case (a duplicated pair, a pair outside the mask)"""
    g = torch.Generator().manual_seed(300 + seed)
    B, S = len(READER_LENS), max(READER_LENS)
    lens = torch.tensor(READER_LENS)
    ar = torch.arange(S)[None]
    mask = ar < lens[:, None]
    ids = torch.randint(1, 120, (B, S), generator=g) * mask
    seg = ((ar >= QUESTION_PART) & mask).long()
    pmask = (ar >= QUESTION_PART) & (ar < lens[:, None] - 1)
    lq = 6
    idq = torch.randint(1, 120, (1, 8), generator=g).expand(B, 8).contiguous()
    mq = (torch.arange(8)[None] < lq).expand(B, 8).contiguous()
    para = (0.4 * torch.randn(N_PARAS, 128, generator=g)).half()
    start = torch.tensor([[7, 7, 12], [6, -1, -1], [2, -1, -1], [-1, -1, -1], [-1, -1, -1]])
    end = torch.tensor([[9, 9, 12], [10, -1, -1], [5, -1, -1], [-1, -1, -1], [-1, -1, -1]])
    labels = torch.zeros(N_PARAS, dtype=torch.long)
    labels[[1, 17, N_PARAS - 1]] = 1
    return {"input_ids": ids, "input_mask": mask, "segment_ids": seg, "paragraph_mask": pmask.long(),
            "input_ids_q": idq * mq, "input_mask_q": mq, "para_embed": para, "top5000_labels": labels,
            "start_positions": start, "end_positions": end, "para_targets": labels[:B].clone()}


SMALL_READER_BATCH = small_reader_batch(0)
