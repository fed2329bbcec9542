"""Trainable dual-tower retriever on MI355X: the towers of proqa_amd.retriever with gradients.

`TrainableRetriever` is a torch.nn.Module with the reference's parameter names (retrieval/retriever.py:10-31), so the
reference's training loop (retrieval/train_retriever.py:196-214) runs with the model class swapped, and the checkpoint it
saves loads into get_embed.py, eval_retrieval.py and train_retriever.py --do_predict unchanged.

Every operator between the dense products is a torch.autograd.Function over a pair of hand-written HIP kernels of
libproqa_hip.so -- the forward operator the inference path uses and its backward (csrc/train_kernels.hip): embedding +
LayerNorm, attention, bias + GELU, bias + residual + LayerNorm, and the in-batch loss.  The forward kernels save
nothing; each backward recomputes what it needs from the forward's inputs, which autograd keeps.

Every linear layer, the pooler and the projection included, is `_Linear`: its weight gradient dW = dY^T X is
proqa_linear_wgrad_f16 (csrc/linear_kernels.hip), fp16 operands summed over all tokens in fp32 in a fixed order and
written as fp32 straight into the buffer whose row slices become the gradients of the masters.  No weight gradient
passes through fp16; a bias gradient is the fp32 column sum of dY.

WHERE TORCH COMPUTES.  The forward products (torch.nn.functional.linear, inside _Linear.forward only) and the input
gradients dX = dY W run on fp16 tensors through the same rocBLAS / hipBLASLt the inference path calls from
csrc/encoder.cpp; so do the pooler's tanh and the casts of the masters.  This file is the one place in proqa_amd/ where
torch computes.  Biases of the encoder layers are NOT passed to linear: the fused operators add them and return their
gradients.

Precision: fp32 master parameters, cast to fp16 once per step and tower (apex O1 semantics; the reference trains with
--fp16), or, after half_weights(), weight matrices whose fp16 working copies the optimizer step writes with the masters; activations and their gradients fp16, every sum inside a kernel fp32, every parameter gradient fp32 (weight
matrices, vectors and embedding tables alike).  Use a loss scale (a fixed one or torch.amp.GradScaler): every backward
operator is linear in its incoming gradient and passes inf / NaN through.

Dropout: transformers' two rates, `hidden_dropout_prob` (embeddings, attention output, FFN output) and
`attention_probs_dropout_prob`, are constructor arguments (default 0: existing callers pass configs that carry 0.1 and
train without).  In train() mode with a rate above 0 the masks live INSIDE the fused operators: each is a pure function of
(seed, site, call, coordinates) (csrc/dropout_rng.h), generated in the forward kernel and again in the backward kernels; no
mask and no [B, heads, S, S] tensor reaches memory.  eval(), and a rate of 0, run exactly the kernels of the
dropout-free path.  There is no CPU path.
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import EMBED_DIM
from .inbatch import block_offsets, inbatch_eval, inbatch_eval_blocks
from .retriever import config_from_dict, tower_keys

_WORKSPACES = {}


def _workspace(device, nbytes):
    """Device scratch of the backward operators: one buffer per device, grown on demand (calls are ordered on the
    current stream)."""
    key = (device.type, device.index)
    t = _WORKSPACES.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WORKSPACES[key] = t
    return t


def _f16(x, name):
    if not x.is_cuda or x.dtype != torch.float16:
        raise ValueError(f"{name} must be a float16 CUDA tensor, got {x.dtype} on {x.device}")
    return x.contiguous()


def _call(fn, dev, *args):
    with torch.cuda.device(dev):
        _lib.check(fn(*args, _lib.current_stream_ptr()))


# ---- the operators, tensor in / tensor out (no autograd) -------------------------------------------------------------------

def colsum(x):
    """[rows, cols] fp16 -> [cols] fp32, rows added in a fixed order (proqa_colsum_f16)."""
    lib = _lib.load()
    x = _f16(x, "x")
    rows, cols = x.shape
    out = torch.empty(cols, dtype=torch.float32, device=x.device)
    ws = _workspace(x.device, lib.proqa_backward_workspace_bytes(cols))
    _call(lib.proqa_colsum_f16, x.device, x.data_ptr(), rows, cols, out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def bias_gelu(x_pre, bias):
    lib = _lib.load()
    x_pre, bias = _f16(x_pre, "x_pre"), _f16(bias, "bias")
    rows, cols = x_pre.shape
    out = torch.empty_like(x_pre)
    _call(lib.proqa_bias_gelu_out_f16, x_pre.device, x_pre.data_ptr(), bias.data_ptr(), rows, cols, out.data_ptr())
    return out


def bias_gelu_backward(dy, x_pre, bias):
    """-> (dx fp16 [rows, cols], dbias fp32 [cols])"""
    lib = _lib.load()
    dy, x_pre, bias = _f16(dy, "dy"), _f16(x_pre, "x_pre"), _f16(bias, "bias")
    rows, cols = x_pre.shape
    dx = torch.empty_like(x_pre)
    dbias = torch.empty(cols, dtype=torch.float32, device=dy.device)
    ws = _workspace(dy.device, lib.proqa_backward_workspace_bytes(cols))
    _call(lib.proqa_bias_gelu_backward_f16, dy.device, dy.data_ptr(), x_pre.data_ptr(), bias.data_ptr(), rows, cols,
          dx.data_ptr(), dbias.data_ptr(), ws.data_ptr(), ws.numel())
    return dx, dbias


def bias_residual_layernorm(x, bias, residual, gamma, beta, eps):
    lib = _lib.load()
    x, residual = _f16(x, "x"), _f16(residual, "residual")
    rows, cols = x.shape
    out = torch.empty_like(x)
    _call(lib.proqa_bias_residual_layernorm_f16, x.device, x.data_ptr(), _f16(bias, "bias").data_ptr(), residual.data_ptr(),
          _f16(gamma, "gamma").data_ptr(), _f16(beta, "beta").data_ptr(), float(eps), rows, cols, out.data_ptr())
    return out


def bias_residual_layernorm_backward(dy, x, bias, residual, gamma, eps):
    """-> (dz fp16 [rows, cols]: the gradient of x and of residual, dgamma, dbeta, dbias fp32 [cols])"""
    lib = _lib.load()
    dy, x, residual = _f16(dy, "dy"), _f16(x, "x"), _f16(residual, "residual")
    bias, gamma = _f16(bias, "bias"), _f16(gamma, "gamma")
    rows, cols = x.shape
    dz = torch.empty_like(x)
    dgamma, dbeta, dbias = (torch.empty(cols, dtype=torch.float32, device=x.device) for _ in range(3))
    ws = _workspace(x.device, lib.proqa_backward_workspace_bytes(cols))
    _call(lib.proqa_bias_residual_layernorm_backward_f16, x.device, dy.data_ptr(), x.data_ptr(), bias.data_ptr(),
          residual.data_ptr(), gamma.data_ptr(), float(eps), rows, cols, dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
          dbias.data_ptr(), ws.data_ptr(), ws.numel())
    return dz, dgamma, dbeta, dbias


def embed_layernorm(ids, cu_seqlens, n_tokens, word, pos, type0, gamma, beta, eps):
    """ids int64 [batch, seq_len] right-padded, cu_seqlens int32 [batch + 1] -> packed [n_tokens, hidden] fp16"""
    lib = _lib.load()
    batch, seq_len = ids.shape
    hidden = word.shape[1]
    out = torch.empty((n_tokens, hidden), dtype=torch.float16, device=ids.device)
    _call(lib.proqa_embed_layernorm_varlen_f16, ids.device, ids.data_ptr(), cu_seqlens.data_ptr(), batch, seq_len, hidden,
          _f16(word, "word").data_ptr(), word.shape[0], _f16(pos, "pos").data_ptr(), _f16(type0, "type0").data_ptr(),
          _f16(gamma, "gamma").data_ptr(), _f16(beta, "beta").data_ptr(), float(eps), out.data_ptr())
    return out


def embed_layernorm_backward(dy, ids, cu_seqlens, word, pos, type0, gamma, eps, deterministic=False):
    """-> fp32 (dgamma [hidden], dbeta [hidden], d_word [vocab, hidden], d_pos [positions, hidden], d_type0 [hidden])
    deterministic: d_word is summed in a fixed order (proqa_embed_layernorm_varlen_backward_det_f16), not with atomics"""
    lib = _lib.load()
    dy = _f16(dy, "dy")
    batch, seq_len = ids.shape
    n_tokens, hidden = dy.shape
    if seq_len > pos.shape[0]:
        raise ValueError(f"sequence length {seq_len} exceeds the {pos.shape[0]} positions of the table")
    dev = dy.device
    dgamma, dbeta, d_type0 = (torch.zeros(hidden, dtype=torch.float32, device=dev) for _ in range(3))
    d_word = torch.zeros(word.shape, dtype=torch.float32, device=dev)
    d_pos = torch.zeros(pos.shape, dtype=torch.float32, device=dev)
    if deterministic:
        fn = lib.proqa_embed_layernorm_varlen_backward_det_f16
        ws = _workspace(dev, lib.proqa_embed_layernorm_backward_det_workspace_bytes(n_tokens, hidden, 0))
    else:
        fn = lib.proqa_embed_layernorm_varlen_backward_f16
        ws = _workspace(dev, lib.proqa_backward_workspace_bytes(hidden))
    _call(fn, dev, dy.data_ptr(), ids.data_ptr(), cu_seqlens.data_ptr(), batch,
          seq_len, hidden, n_tokens, _f16(word, "word").data_ptr(), word.shape[0], _f16(pos, "pos").data_ptr(),
          _f16(type0, "type0").data_ptr(), _f16(gamma, "gamma").data_ptr(), float(eps), dgamma.data_ptr(), dbeta.data_ptr(),
          d_word.data_ptr(), d_pos.data_ptr(), d_type0.data_ptr(), ws.data_ptr(), ws.numel())
    return dgamma, dbeta, d_word, d_pos, d_type0


def embed_layernorm_typed(ids, type_ids, cu_seqlens, n_tokens, word, pos, types, gamma, beta, eps):
    """embed_layernorm with token types: type_ids int64 [batch, seq_len] like ids (None: all 0), types [n_types, hidden]"""
    lib = _lib.load()
    batch, seq_len = ids.shape
    hidden = word.shape[1]
    out = torch.empty((n_tokens, hidden), dtype=torch.float16, device=ids.device)
    _call(lib.proqa_embed_layernorm_typed_varlen_f16, ids.device, ids.data_ptr(), type_ids.data_ptr() if type_ids is not None
          else None, cu_seqlens.data_ptr(), batch, seq_len, hidden, _f16(word, "word").data_ptr(), word.shape[0],
          _f16(pos, "pos").data_ptr(), _f16(types, "types").data_ptr(), types.shape[0], _f16(gamma, "gamma").data_ptr(),
          _f16(beta, "beta").data_ptr(), float(eps), out.data_ptr())
    return out


def embed_layernorm_typed_backward(dy, ids, type_ids, cu_seqlens, word, pos, types, gamma, eps, deterministic=False):
    """-> fp32 (dgamma [hidden], dbeta [hidden], d_word [vocab, hidden], d_pos [positions, hidden], d_types [n_types, hidden])
    deterministic: d_word is summed in a fixed order (proqa_embed_layernorm_typed_varlen_backward_det_f16)"""
    lib = _lib.load()
    dy = _f16(dy, "dy")
    batch, seq_len = ids.shape
    n_tokens, hidden = dy.shape
    if seq_len > pos.shape[0]:
        raise ValueError(f"sequence length {seq_len} exceeds the {pos.shape[0]} positions of the table")
    if type_ids is not None and type_ids.shape != ids.shape:
        raise ValueError(f"type_ids {tuple(type_ids.shape)} must have the shape of ids {tuple(ids.shape)}")
    dev = dy.device
    dgamma, dbeta = (torch.zeros(hidden, dtype=torch.float32, device=dev) for _ in range(2))
    d_word = torch.zeros(word.shape, dtype=torch.float32, device=dev)
    d_pos = torch.zeros(pos.shape, dtype=torch.float32, device=dev)
    d_types = torch.zeros(types.shape, dtype=torch.float32, device=dev)
    if deterministic:
        fn = lib.proqa_embed_layernorm_typed_varlen_backward_det_f16
        ws = _workspace(dev, lib.proqa_embed_layernorm_backward_det_workspace_bytes(n_tokens, hidden, 1))
    else:
        fn = lib.proqa_embed_layernorm_typed_varlen_backward_f16
        ws = _workspace(dev, lib.proqa_embed_layernorm_typed_backward_workspace_bytes(hidden))
    _call(fn, dev, dy.data_ptr(), ids.data_ptr(),
          type_ids.data_ptr() if type_ids is not None else None, cu_seqlens.data_ptr(), batch, seq_len, hidden, n_tokens,
          _f16(word, "word").data_ptr(), word.shape[0], _f16(pos, "pos").data_ptr(), _f16(types, "types").data_ptr(),
          types.shape[0], _f16(gamma, "gamma").data_ptr(), float(eps), dgamma.data_ptr(), dbeta.data_ptr(), d_word.data_ptr(),
          d_pos.data_ptr(), d_types.data_ptr(), ws.data_ptr(), ws.numel())
    return dgamma, dbeta, d_word, d_pos, d_types


def attention(qkv, qkv_bias, cu_seqlens, batch, max_seq_len, n_heads):
    """qkv packed [T, 3*hidden] fp16 (before the bias), qkv_bias [3*hidden] fp16 or None -> ctx [T, hidden]"""
    lib = _lib.load()
    qkv = _f16(qkv, "qkv")
    out = torch.empty((qkv.shape[0], n_heads * 64), dtype=torch.float16, device=qkv.device)
    _call(lib.proqa_attention_ex_f16, qkv.device, qkv.data_ptr(), _f16(qkv_bias, "qkv_bias").data_ptr() if qkv_bias is not None
          else None, None, cu_seqlens.data_ptr(), batch, max_seq_len, n_heads, 0, out.data_ptr())
    return out


def attention_backward(qkv, qkv_bias, d_ctx, cu_seqlens, batch, max_seq_len, n_heads):
    """-> d_qkv [T, 3*hidden] fp16; the gradient of qkv_bias is colsum(d_qkv)"""
    lib = _lib.load()
    qkv, d_ctx = _f16(qkv, "qkv"), _f16(d_ctx, "d_ctx")
    n_tokens = qkv.shape[0]
    if qkv.shape[1] != 3 * n_heads * 64 or d_ctx.shape != (n_tokens, n_heads * 64):
        raise ValueError(f"attention_backward: qkv {tuple(qkv.shape)} / d_ctx {tuple(d_ctx.shape)} do not fit {n_heads} heads of 64")
    d_qkv = torch.empty_like(qkv)
    ws = _workspace(qkv.device, lib.proqa_attention_backward_workspace_bytes(n_tokens, n_heads))
    _call(lib.proqa_attention_backward_f16, qkv.device, qkv.data_ptr(), _f16(qkv_bias, "qkv_bias").data_ptr() if qkv_bias is not None
          else None, d_ctx.data_ptr(), cu_seqlens.data_ptr(), batch, max_seq_len, n_heads, n_tokens, d_qkv.data_ptr(),
          ws.data_ptr(), ws.numel())
    return d_qkv


# ---- the operators with dropout.  `drop` = (p, seed, site, call) as Python numbers; p == 0 is the dropout-free operator itself.

def _drop_args(drop):
    p, seed, site, call = drop
    return float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(site), int(call) & 0xFFFFFF


def dropout(x, drop):
    """x [rows, cols] fp16 -> x * keep / (1 - p_eff) (proqa_dropout_f16); its backward is the same call on dy"""
    lib = _lib.load()
    x = _f16(x, "x")
    if drop[0] == 0:
        return x.clone()
    rows, cols = x.shape
    out = torch.empty_like(x)
    p, seed, site, call = _drop_args(drop)
    _call(lib.proqa_dropout_f16, x.device, x.data_ptr(), rows, cols, p, seed, site, call, out.data_ptr())
    return out


def bias_residual_layernorm_dropout(x, bias, residual, gamma, beta, eps, drop):
    """LayerNorm(dropout(x + bias) + residual)"""
    if drop[0] == 0:
        return bias_residual_layernorm(x, bias, residual, gamma, beta, eps)
    lib = _lib.load()
    x, residual = _f16(x, "x"), _f16(residual, "residual")
    rows, cols = x.shape
    out = torch.empty_like(x)
    p, seed, site, call = _drop_args(drop)
    _call(lib.proqa_bias_residual_layernorm_dropout_f16, x.device, x.data_ptr(), _f16(bias, "bias").data_ptr(),
          residual.data_ptr(), _f16(gamma, "gamma").data_ptr(), _f16(beta, "beta").data_ptr(), float(eps), rows, cols,
          p, seed, site, call, out.data_ptr())
    return out


def bias_residual_layernorm_dropout_backward(dy, x, bias, residual, gamma, eps, drop):
    """-> (dx fp16, dresidual fp16 [rows, cols], dgamma, dbeta, dbias fp32 [cols])"""
    if drop[0] == 0:
        dz, dgamma, dbeta, dbias = bias_residual_layernorm_backward(dy, x, bias, residual, gamma, eps)
        return dz, dz, dgamma, dbeta, dbias
    lib = _lib.load()
    dy, x, residual = _f16(dy, "dy"), _f16(x, "x"), _f16(residual, "residual")
    bias, gamma = _f16(bias, "bias"), _f16(gamma, "gamma")
    rows, cols = x.shape
    dx, dres = torch.empty_like(x), torch.empty_like(x)
    dgamma, dbeta, dbias = (torch.empty(cols, dtype=torch.float32, device=x.device) for _ in range(3))
    ws = _workspace(x.device, lib.proqa_backward_workspace_bytes(cols))
    p, seed, site, call = _drop_args(drop)
    _call(lib.proqa_bias_residual_layernorm_dropout_backward_f16, x.device, dy.data_ptr(), x.data_ptr(), bias.data_ptr(),
          residual.data_ptr(), gamma.data_ptr(), float(eps), rows, cols, p, seed, site, call, dx.data_ptr(), dres.data_ptr(),
          dgamma.data_ptr(), dbeta.data_ptr(), dbias.data_ptr(), ws.data_ptr(), ws.numel())
    return dx, dres, dgamma, dbeta, dbias


def attention_dropout(qkv, qkv_bias, cu_seqlens, batch, max_seq_len, n_heads, drop):
    """attention() with the probabilities dropped (proqa_attention_dropout_f16)"""
    if drop[0] == 0:
        return attention(qkv, qkv_bias, cu_seqlens, batch, max_seq_len, n_heads)
    lib = _lib.load()
    qkv = _f16(qkv, "qkv")
    out = torch.empty((qkv.shape[0], n_heads * 64), dtype=torch.float16, device=qkv.device)
    p, seed, site, call = _drop_args(drop)
    _call(lib.proqa_attention_dropout_f16, qkv.device, qkv.data_ptr(), _f16(qkv_bias, "qkv_bias").data_ptr() if qkv_bias is not None
          else None, cu_seqlens.data_ptr(), batch, max_seq_len, n_heads, p, seed, site, call, out.data_ptr())
    return out


def attention_dropout_backward(qkv, qkv_bias, d_ctx, cu_seqlens, batch, max_seq_len, n_heads, drop):
    """-> d_qkv [T, 3*hidden] fp16; the gradient of qkv_bias is colsum(d_qkv)"""
    if drop[0] == 0:
        return attention_backward(qkv, qkv_bias, d_ctx, cu_seqlens, batch, max_seq_len, n_heads)
    lib = _lib.load()
    qkv, d_ctx = _f16(qkv, "qkv"), _f16(d_ctx, "d_ctx")
    n_tokens = qkv.shape[0]
    if qkv.shape[1] != 3 * n_heads * 64 or d_ctx.shape != (n_tokens, n_heads * 64):
        raise ValueError(f"attention_dropout_backward: qkv {tuple(qkv.shape)} / d_ctx {tuple(d_ctx.shape)} do not fit {n_heads} heads of 64")
    d_qkv = torch.empty_like(qkv)
    ws = _workspace(qkv.device, lib.proqa_attention_backward_workspace_bytes(n_tokens, n_heads))
    p, seed, site, call = _drop_args(drop)
    _call(lib.proqa_attention_dropout_backward_f16, qkv.device, qkv.data_ptr(), _f16(qkv_bias, "qkv_bias").data_ptr()
          if qkv_bias is not None else None, d_ctx.data_ptr(), cu_seqlens.data_ptr(), batch, max_seq_len, n_heads, n_tokens,
          p, seed, site, call, d_qkv.data_ptr(), ws.data_ptr(), ws.numel())
    return d_qkv


def linear_wgrad(dy, x, out=None, accumulate=False):
    """dw [N, K] fp32 = (out if accumulate else 0) + dy^T x: dy [T, N], x [T, K] fp16 (proqa_linear_wgrad_f16).  The sum
    over the T tokens is one fp32 sum in a fixed order; nothing passes through fp16.  out: a contiguous fp32 [N, K]
    tensor to write or add into (required when accumulate is set)."""
    lib = _lib.load()
    dy, x = _f16(dy, "dy"), _f16(x, "x")
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != x.shape[0]:
        raise ValueError(f"linear_wgrad: dy {tuple(dy.shape)} and x {tuple(x.shape)} must be [T, N] and [T, K]")
    (T, N), K = dy.shape, x.shape[1]
    if out is None:
        if accumulate:
            raise ValueError("linear_wgrad: accumulate needs an `out` to add into")
        out = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    elif out.dtype != torch.float32 or out.shape != (N, K) or not out.is_contiguous() or out.device != dy.device:
        raise ValueError(f"linear_wgrad: out must be a contiguous float32 [{N}, {K}] tensor on {dy.device}")
    splits, need = ctypes.c_int(0), ctypes.c_size_t(0)
    n_cus = torch.cuda.get_device_properties(dy.device).multi_processor_count
    _lib.check(lib.proqa_linear_wgrad_plan(T, N, K, n_cus, ctypes.byref(splits), ctypes.byref(need)))
    ws = _workspace(dy.device, need.value)
    _call(lib.proqa_linear_wgrad_f16, dy.device, dy.data_ptr(), x.data_ptr(), T, N, K, out.data_ptr(), int(bool(accumulate)),
          ws.data_ptr(), ws.numel())
    return out


def inbatch_loss_grad(q, c, target, lse, grad_in):
    """Gradient of mean_i (lse_i - s[i, target_i]) times the device scalar grad_in -> (dq, dc) fp16"""
    lib = _lib.load()
    q, c = _f16(q, "q"), _f16(c, "c")
    t = None if target is None else target.to(device=q.device, dtype=torch.int32).contiguous()
    lse = lse.to(torch.float32).contiguous()
    g = grad_in.to(device=q.device, dtype=torch.float32).reshape(1).contiguous()
    dq, dc = torch.empty_like(q), torch.empty_like(c)
    _call(lib.proqa_inbatch_loss_grad_f16, q.device, q.data_ptr(), c.data_ptr(), t.data_ptr() if t is not None else None,
          lse.data_ptr(), g.data_ptr(), q.shape[0], c.shape[0], q.shape[1], dq.data_ptr(), dc.data_ptr())
    return dq, dc


def inbatch_loss_blocks_grad(q, c, offsets, lse, grad_in):
    """Gradient of sum_m grad_in[m] * loss_m of the block-diagonal objective (offsets: inbatch.block_offsets(); lse as
    inbatch_eval_blocks wrote it; grad_in: device fp32 [M]) -> (dq, dc) fp16"""
    lib = _lib.load()
    q, c = _f16(q, "q"), _f16(c, "c")
    M = len(offsets) - 1
    lse = lse.to(torch.float32).contiguous()
    g = grad_in.to(device=q.device, dtype=torch.float32).contiguous()
    if g.shape != (M,) or lse.shape != (q.shape[0],) or c.shape != q.shape:
        raise ValueError(f"inbatch_loss_blocks_grad: grad_in {tuple(g.shape)} / lse {tuple(lse.shape)} / c {tuple(c.shape)} "
                         f"do not fit {M} blocks over q {tuple(q.shape)}")
    dq, dc = torch.empty_like(q), torch.empty_like(c)
    _call(lib.proqa_inbatch_loss_blocks_grad_f16, q.device, q.data_ptr(), c.data_ptr(), offsets, M, q.shape[0], q.shape[1],
          lse.data_ptr(), g.data_ptr(), dq.data_ptr(), dc.data_ptr())
    return dq, dc


# ---- autograd: each forward operator with its backward ---------------------------------------------------------------------
# Parameters enter as the fp32 masters and are cast inside forward, so that their gradients leave as fp32.

class _EmbedLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, cu_seqlens, n_tokens, word, pos, types, gamma, beta, eps, deterministic=False):
        w16, p16, t16, g16 = word.half(), pos.half(), types[0].half().contiguous(), gamma.half()
        ctx.save_for_backward(ids, cu_seqlens, w16, p16, t16, g16)
        ctx.eps, ctx.n_types, ctx.deterministic = eps, types.shape[0], bool(deterministic)
        return embed_layernorm(ids, cu_seqlens, n_tokens, w16, p16, t16, g16, beta.half(), eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        ids, cu, w16, p16, t16, g16 = ctx.saved_tensors
        dgamma, dbeta, d_word, d_pos, d_type0 = embed_layernorm_backward(dy, ids, cu, w16, p16, t16, g16, ctx.eps,
                                                                         ctx.deterministic)
        d_types = torch.zeros((ctx.n_types, d_type0.shape[0]), dtype=torch.float32, device=dy.device)
        d_types[0] = d_type0          # token_type_ids are never passed: row 0 only
        return None, None, None, d_word, d_pos, d_types, dgamma, dbeta, None, None


class _EmbedLayerNormTyped(torch.autograd.Function):
    """The reader's embeddings: token types from `type_ids`; the gradient of the type table is the full [n_types, hidden]."""

    @staticmethod
    def forward(ctx, ids, type_ids, cu_seqlens, n_tokens, word, pos, types, gamma, beta, eps, deterministic=False):
        w16, p16, t16, g16 = word.half(), pos.half(), types.half().contiguous(), gamma.half()
        ctx.save_for_backward(ids, type_ids, cu_seqlens, w16, p16, t16, g16)
        ctx.eps, ctx.deterministic = eps, bool(deterministic)
        return embed_layernorm_typed(ids, type_ids, cu_seqlens, n_tokens, w16, p16, t16, g16, beta.half(), eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        ids, type_ids, cu, w16, p16, t16, g16 = ctx.saved_tensors
        dgamma, dbeta, d_word, d_pos, d_types = embed_layernorm_typed_backward(dy, ids, type_ids, cu, w16, p16, t16, g16, ctx.eps,
                                                                               ctx.deterministic)
        return None, None, None, None, d_word, d_pos, d_types, dgamma, dbeta, None, None


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, drop):
        ctx.drop = drop
        return dropout(x, drop)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        return dropout(dy, ctx.drop), None


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, qkv_bias, cu_seqlens, batch, max_seq_len, n_heads, drop=None):
        b16 = qkv_bias.half()
        ctx.save_for_backward(qkv, b16, cu_seqlens)
        ctx.dims = (batch, max_seq_len, n_heads)
        ctx.drop = drop
        if drop is None:
            return attention(qkv, b16, cu_seqlens, batch, max_seq_len, n_heads)
        return attention_dropout(qkv, b16, cu_seqlens, batch, max_seq_len, n_heads, drop)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_ctx):
        qkv, b16, cu = ctx.saved_tensors
        if ctx.drop is None:
            d_qkv = attention_backward(qkv, b16, d_ctx, cu, *ctx.dims)
        else:
            d_qkv = attention_dropout_backward(qkv, b16, d_ctx, cu, *ctx.dims, ctx.drop)
        return d_qkv, colsum(d_qkv), None, None, None, None, None


class _BiasGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_pre, bias):
        b16 = bias.half()
        ctx.save_for_backward(x_pre, b16)
        return bias_gelu(x_pre, b16)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x_pre, b16 = ctx.saved_tensors
        return bias_gelu_backward(dy, x_pre, b16)


class _BiasResidualLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, residual, gamma, beta, eps, drop=None):
        b16, g16 = bias.half(), gamma.half()
        ctx.save_for_backward(x, b16, residual, g16)
        ctx.eps, ctx.drop = eps, drop
        if drop is None:
            return bias_residual_layernorm(x, b16, residual, g16, beta.half(), eps)
        return bias_residual_layernorm_dropout(x, b16, residual, g16, beta.half(), eps, drop)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, b16, residual, g16 = ctx.saved_tensors
        if ctx.drop is None:
            dz, dgamma, dbeta, dbias = bias_residual_layernorm_backward(dy, x, b16, residual, g16, ctx.eps)
            return dz, dbias, dz, dgamma, dbeta, None, None
        dx, dres, dgamma, dbeta, dbias = bias_residual_layernorm_dropout_backward(dy, x, b16, residual, g16, ctx.eps, ctx.drop)
        return dx, dbias, dres, dgamma, dbeta, None, None


class _Linear(torch.autograd.Function):
    """y = x [w_0; w_1; ...]^T (+ bias) over the fp32 masters w_i [N_i, K]: the Q / K / V layer is three masters and one
    product.  The forward and dx = dy w go through torch (rocBLAS / hipBLASLt); the weight gradient is linear_wgrad, one
    call into an fp32 [sum N_i, K] buffer whose row slices are the gradients of the masters.
    w16: the fp16 working copy [sum N_i, K] that the optimizer step keeps current (half_weights), taken as it lies, or None:
    the masters are cast here, one copy_ per master."""

    @staticmethod
    def forward(ctx, x, bias, w16, *weights):
        if w16 is None:
            w16 = torch.empty((sum(w.shape[0] for w in weights), weights[0].shape[1]), dtype=torch.float16, device=x.device)
            r = 0
            for w in weights:
                w16[r:r + w.shape[0]].copy_(w)         # the cast, straight into its row slice
                r += w.shape[0]
        ctx.save_for_backward(x, w16)
        ctx.rows = [w.shape[0] for w in weights]
        return F.linear(x, w16, bias.half() if bias is not None else None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w16 = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy = dy.contiguous()
        dx = dy @ w16 if need[0] else None
        dbias = colsum(dy) if need[1] else None
        dws = [None] * len(ctx.rows)
        if any(need[3:]):
            dw = linear_wgrad(dy, x)
            r = 0
            for i, n in enumerate(ctx.rows):
                if need[3 + i]:
                    dws[i] = dw[r:r + n]
                r += n
        return (dx, dbias, None, *dws)


class _InBatchLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, c, target):
        out = inbatch_eval(q, c, target)
        ctx.save_for_backward(q, c, out["lse"])
        ctx.target = target
        return (out["lse"] - out["gold"]).mean()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        q, c, lse = ctx.saved_tensors
        dq, dc = inbatch_loss_grad(q, c, ctx.target, lse, grad_out)
        return dq, dc, None


def inbatch_loss(q, c, target=None):
    """CrossEntropyLoss(q @ c.T, target) (target None: arange) as an fp32 scalar with gradients, without the [nq, nc]
    product in memory: the forward value is proqa_inbatch_eval_f16's mean(lse - gold), the backward
    proqa_inbatch_loss_grad_f16.  q, c: fp16 [n, 128] device tensors."""
    return _InBatchLoss.apply(q, c, target)


class _InBatchLossBlocks(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, c, offsets):
        out = inbatch_eval_blocks(q, c, offsets)
        ctx.save_for_backward(q, c, out["lse"])
        ctx.offsets = offsets
        return out["loss"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        q, c, lse = ctx.saved_tensors
        dq, dc = inbatch_loss_blocks_grad(q, c, ctx.offsets, lse, grad_out)
        return dq, dc, None


def inbatch_loss_blocks(q, c, block_sizes):
    """The block-diagonal in-batch objective: block m owns the next block_sizes[m] rows of BOTH q and c [n, 128] fp16, and
    its loss is CrossEntropyLoss(q_m @ c_m.T, arange) -- what inbatch_loss(q_m, c_m) gives per block, in one call
    (proqa_inbatch_loss_blocks_f16, backward proqa_inbatch_loss_blocks_grad_f16) -> fp32 [M] with gradients.  One autograd
    node; torch computes nothing in it.  For a block of at most 512 rows the gradients carry the bits of the per-block
    calls (proqa_hip.h)."""
    return _InBatchLossBlocks.apply(q, c, block_offsets(block_sizes, q.shape[0]))


# ---- one tower pass, shared by TrainableRetriever and TrainableReader ----------------------------------------------------------

def run_tower(P, tower, cfg, input_ids, input_mask, *, type_ids=None, proj=None, drop=(0.0, 0.0, 0, 0), probe_extra=None,
              half=None, seq_lens_host=None, deterministic=False):
    """One BERT tower with gradients.  P: {key: fp32 master}; `tower` the key prefix of the tower's parameters (bert_q,
    bert_c, bert).  input_ids / input_mask [B, S] right-padded CUDA tensors, B >= 1; type_ids [B, S] or None (every token
    of type 0: the untyped embedding operator).  drop = (hidden rate, attention rate, seed, call) of this pass; a rate of 0
    runs the dropout-free operator.  probe_extra(lens) -> (device bool scalar, message): one more condition for the pass's
    single host round trip to check (ValueError(message) when it holds).  half: {tuple of weight keys: fp16 working copy
    of those masters stacked by rows} for EVERY product of the pass (HalfWeights.views), or None: each product casts its
    masters itself.  seq_lens_host: the rows' lengths as a list of B ints that the caller vouches for (the mask is a
    prefix of that many ones per row): the pass then makes NO host round trip -- the mask is not read or checked, and
    probe_extra must be None.  deterministic: the word-embedding gradient is summed in a fixed order (DESIGN.md section 3e,
    Determinism) and not with atomics, so that every gradient of the pass is bit-identical from run to run.
    -> proj given (the key prefix of the projection): the [B, 128] fp16 embedding of pooler + projection;
       proj None: (h, cu_seqlens, lens, max_len), the packed last hidden state [T, H] fp16 and its geometry."""
    B, S = input_ids.shape
    if S > cfg.max_position_embeddings or S > 512:
        raise ValueError(f"sequence length {S} exceeds max_position_embeddings {cfg.max_position_embeddings} (or 512)")
    ids = input_ids.contiguous().to(torch.int64)
    mask = input_mask.to(torch.bool)
    # as BertForRetriever.encode: a row without a valid token is evaluated as its first token; the mask of every row
    # must be a prefix of ones (re_collate pads on the right); one host round trip for the check and the sizes
    if seq_lens_host is not None:
        host = [int(n) for n in seq_lens_host]
        if probe_extra is not None or len(host) != B or not all(1 <= n <= S for n in host):
            raise ValueError(f"seq_lens_host must be {B} lengths in [1, {S}] (and excludes probe_extra)")
        if len(set(host)) == 1:          # one length (a single question): a fill on the device, nothing is copied up
            lens = torch.full((B,), host[0], dtype=torch.int32, device=ids.device)
        else:
            lens = torch.tensor(host, dtype=torch.int32).to(ids.device)
        n_tokens, max_len = sum(host), max(host)
    else:
        lens = mask.sum(dim=1).clamp_(min=1).to(torch.int32)
        bad = (mask[:, 1:] & ~mask[:, :-1]).any() if S > 1 else torch.zeros((), dtype=torch.bool, device=mask.device)
        flags = [bad.to(torch.int64), lens.sum(dtype=torch.int64), lens.max().to(torch.int64)]
        extra_message = None
        if probe_extra is not None:
            extra_bad, extra_message = probe_extra(lens)
            flags.append(extra_bad.to(torch.int64))
        probe = torch.stack(flags).cpu()
        if bool(probe[0]):
            raise ValueError("input_mask must be right-padded (a prefix of True per row), as re_collate produces")
        if extra_message is not None and bool(probe[3]):
            raise ValueError(extra_message)
        n_tokens, max_len = int(probe[1]), int(probe[2])
    cu = torch.zeros(B + 1, dtype=torch.int32, device=ids.device)
    cu[1:] = torch.cumsum(lens, 0)
    eps, n_heads = float(cfg.layer_norm_eps), cfg.num_attention_heads
    # a site whose rate is 0 (or eval()) gets None and runs the dropout-free operator
    p_hid, p_att, seed, call = drop
    hid = (lambda site: (p_hid, seed, site, call)) if p_hid > 0 else (lambda site: None)
    att = (lambda site: (p_att, seed, site, call)) if p_att > 0 else (lambda site: None)

    def linear(x, bias, *keys):
        return _Linear.apply(x, bias, half[keys] if half is not None else None, *(P[k] for k in keys))

    e = f"{tower}.embeddings"
    tables = (P[f"{e}.word_embeddings.weight"], P[f"{e}.position_embeddings.weight"], P[f"{e}.token_type_embeddings.weight"],
              P[f"{e}.LayerNorm.weight"], P[f"{e}.LayerNorm.bias"])
    if type_ids is None:
        h = _EmbedLayerNorm.apply(ids, cu, n_tokens, *tables, eps, deterministic)
    else:
        h = _EmbedLayerNormTyped.apply(ids, type_ids.contiguous().to(torch.int64), cu, n_tokens, *tables, eps, deterministic)
    if p_hid > 0:
        h = _Dropout.apply(h, hid(0))
    for i in range(cfg.num_hidden_layers):
        p = f"{tower}.encoder.layer.{i}"
        qkv_b = torch.cat([P[f"{p}.attention.self.{n}.bias"] for n in ("query", "key", "value")], 0)
        qkv = linear(h, None, *(f"{p}.attention.self.{n}.weight" for n in ("query", "key", "value")))
        ctx = _Attention.apply(qkv, qkv_b, cu, B, max_len, n_heads, att(1 + 3 * i))
        a = linear(ctx, None, f"{p}.attention.output.dense.weight")
        h1 = _BiasResidualLayerNorm.apply(a, P[f"{p}.attention.output.dense.bias"], h,
                                          P[f"{p}.attention.output.LayerNorm.weight"],
                                          P[f"{p}.attention.output.LayerNorm.bias"], eps, hid(2 + 3 * i))
        f = _BiasGelu.apply(linear(h1, None, f"{p}.intermediate.dense.weight"), P[f"{p}.intermediate.dense.bias"])
        o = linear(f, None, f"{p}.output.dense.weight")
        h = _BiasResidualLayerNorm.apply(o, P[f"{p}.output.dense.bias"], h1, P[f"{p}.output.LayerNorm.weight"],
                                         P[f"{p}.output.LayerNorm.bias"], eps, hid(3 + 3 * i))
    if proj is None:
        return h, cu, lens, max_len
    cls = h.index_select(0, cu[:-1].to(torch.int64))
    pooled = torch.tanh(linear(cls, P[f"{tower}.pooler.dense.bias"], f"{tower}.pooler.dense.weight"))
    return linear(pooled, P[f"{proj}.bias"], f"{proj}.weight")


# ---- fp16 working copies of the weight matrices, kept current by the optimizer step ------------------------------------------

_COPY_ALIGN = 128        # elements: every copy starts on a 256-byte boundary of the flat buffer (16 bytes are required)


def linear_groups(tower, cfg, proj=None):
    """The weight keys of each product of run_tower(tower, proj=proj), in the pass's order: the Q / K / V masters of a
    layer form one group (one product over their rows), every other matrix its own."""
    groups = []
    for i in range(cfg.num_hidden_layers):
        p = f"{tower}.encoder.layer.{i}"
        groups.append(tuple(f"{p}.attention.self.{n}.weight" for n in ("query", "key", "value")))
        groups += [(f"{p}.attention.output.dense.weight",), (f"{p}.intermediate.dense.weight",), (f"{p}.output.dense.weight",)]
    if proj is not None:
        groups += [(f"{tower}.pooler.dense.weight",), (f"{proj}.weight",)]
    return groups


class HalfWeights:
    """One flat fp16 buffer with a working copy of every weight matrix of `groups` (linear_groups): the masters of a group
    lie adjacent in the group's order, so that the group's product takes one [sum N_i, K] view.
    .views   {group: fp16 [sum N_i, K] view}: what run_tower(half=...) takes
    .copies  {parameter: fp16 view of its shape}: what FusedAdamW(half_copies=...) takes
    The buffer is filled by refresh() (proqa_cast_half_tensors) and from then on by the optimizer step."""

    def __init__(self, P, groups):
        self._params = [P[k] for group in groups for k in group]
        dev = self._params[0].device
        offsets, at = [], 0
        for group in groups:
            at = -(-at // _COPY_ALIGN) * _COPY_ALIGN
            offsets.append(at)
            at += sum(P[k].numel() for k in group)
        self.flat = torch.empty(at, dtype=torch.float16, device=dev)
        self.views, self.copies = {}, {}
        for group, start in zip(groups, offsets):
            K = P[group[0]].shape[1]
            rows = sum(P[k].shape[0] for k in group)
            self.views[group] = self.flat[start:start + rows * K].view(rows, K)
            for k in group:
                self.copies[P[k]] = self.flat[start:start + P[k].numel()].view(P[k].shape)
                start += P[k].numel()
        self._pointers = [p.data_ptr() for p in self._params]
        self.refresh()

    def moved(self):
        """True when a master no longer lies where its copy was made from (an _apply that moved storage)"""
        return [p.data_ptr() for p in self._params] != self._pointers

    def refresh(self):
        """copy = (fp16) master for every matrix: one launch"""
        from .optim import cast_half_tensors
        cast_half_tensors(self._params, [self.copies[p] for p in self._params])


# ---- the module -----------------------------------------------------------------------------------------------------------

def state_dict_keys(config):
    """The reference checkpoint's keys (BertForRetriever.state_dict_keys), without a GPU."""
    cfg = config if not isinstance(config, dict) else config_from_dict(config)
    n = cfg.num_hidden_layers
    return (tower_keys("bert_q", n) + tower_keys("bert_c", n) + ["proj_q.weight", "proj_q.bias", "proj_c.weight", "proj_c.bias"])


def _parameter_shapes(cfg, keys=None):
    """{key: shape} of the tower / projection parameters `keys` (default: the retriever's state_dict_keys)"""
    H, I = cfg.hidden_size, cfg.intermediate_size
    shapes = {}
    for key in (state_dict_keys(cfg) if keys is None else keys):
        if key.startswith("proj_"):
            shapes[key] = (EMBED_DIM, H) if key.endswith("weight") else (EMBED_DIM,)
        elif "word_embeddings" in key:
            shapes[key] = (cfg.vocab_size, H)
        elif "position_embeddings" in key:
            shapes[key] = (cfg.max_position_embeddings, H)
        elif "token_type_embeddings" in key:
            shapes[key] = (cfg.type_vocab_size, H)
        elif "LayerNorm" in key:
            shapes[key] = (H,)
        elif "intermediate.dense" in key:
            shapes[key] = (I, H) if key.endswith("weight") else (I,)
        elif ".output.dense.weight" in key and "attention" not in key:
            shapes[key] = (H, I)
        else:
            shapes[key] = (H, H) if key.endswith("weight") else (H,)
    return shapes


def _cat_right_padded(xs):
    """[B_i, S_i] tensors -> [sum B_i, max S_i], zeros (padding id, mask False) on the right"""
    S = max(x.shape[1] for x in xs)
    if all(x.shape[1] == S for x in xs):
        return torch.cat(xs, 0)
    out = xs[0].new_zeros((sum(x.shape[0] for x in xs), S))
    r = 0
    for x in xs:
        out[r:r + x.shape[0], :x.shape[1]] = x
        r += x.shape[0]
    return out


class _Node(torch.nn.Module):
    """A container: the dotted reference names are paths through these."""


class TrainableRetriever(torch.nn.Module):
    """BertForRetriever with gradients.  forward(batch) takes a re_collate batch (input_ids_q / input_mask_q / input_ids_c /
    input_mask_c, right-padded) and returns {'q': [B, 128], 'c': [B, 128]} in fp16 with gradients."""

    def __init__(self, config, device=None, dropout=0.0, *, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                 dropout_seed=None, deterministic=False):
        super().__init__()
        cfg = config if not isinstance(config, dict) else config_from_dict(config)
        if dropout != 0:
            raise ValueError("TrainableRetriever has no single dropout rate; dropout must be 0: pass BERT's two rates as "
                             "hidden_dropout_prob= and attention_probs_dropout_prob= (DESIGN.md section 3e)")
        for name, rate in (("hidden_dropout_prob", hidden_dropout_prob), ("attention_probs_dropout_prob", attention_probs_dropout_prob)):
            if not 0.0 <= float(rate) <= 0.9:
                raise ValueError(f"{name}={rate!r}: a dropout rate must be in [0, 0.9]")
        dev = torch.device(device) if device is not None else torch.device("cuda")
        if dev.type != "cuda":
            raise RuntimeError("proqa_amd.TrainableRetriever runs on MI355X only; there is no CPU path")
        if cfg.hidden_size != cfg.num_attention_heads * 64:
            raise ValueError("the attention kernels are built for head_dim 64 (bert-base/large geometry)")
        if getattr(cfg, "hidden_act", "gelu") != "gelu":
            raise ValueError("only hidden_act='gelu' (erf) is implemented, as in bert-base-uncased")
        if cfg.hidden_size > 1024 or cfg.intermediate_size > 8192:
            raise ValueError("hidden_size <= 1024 and intermediate_size <= 8192")
        _lib.load()
        _lib.require_gpu()
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.config = cfg
        self.device = dev
        self.hidden_dropout_prob = float(hidden_dropout_prob)
        self.attention_probs_dropout_prob = float(attention_probs_dropout_prob)
        self.deterministic = bool(deterministic)     # the word-embedding gradient in a fixed order (no atomics)
        # the masks' (seed, call): plain Python numbers, not part of state_dict() (which keeps the reference's keys)
        self._dropout_seed = int(torch.initial_seed() if dropout_seed is None else dropout_seed) & 0xFFFFFFFFFFFFFFFF
        self._dropout_call = 0
        self._half = None           # HalfWeights once half_weights() was called
        self._flat = {}
        g = torch.Generator().manual_seed(0)
        for key, shape in _parameter_shapes(cfg).items():      # transformers' initialisation: N(0, 0.02), LayerNorm (1, 0), biases 0
            if key.endswith("LayerNorm.weight"):
                value = torch.ones(shape)
            elif key.endswith(".bias"):
                value = torch.zeros(shape)
            else:
                value = 0.02 * torch.randn(shape, generator=g)
            node = self
            *path, leaf = key.split(".")
            for name in path:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            p = torch.nn.Parameter(value.to(dev))
            node.register_parameter(leaf, p)
            self._flat[key] = p

    # -- reference-compatible surface -----------------------------------------------------
    def state_dict_keys(self):
        return state_dict_keys(self.config)

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """Accepts the reference checkpoint layout: a 'module.' prefix (DataParallel) is stripped, `position_ids` buffers
        of newer transformers are ignored."""
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        sd = {k: v for k, v in sd.items() if not k.endswith("position_ids")}
        result = super().load_state_dict(sd, strict=strict, **kwargs)
        self.refresh_half_weights()
        return result

    def half_weights(self):
        """Switch the module to fp16 working copies of its weight matrices and return {parameter: fp16 view} for
        FusedAdamW(half_copies=...), whose step then writes each copy with the master.  One flat buffer, every copy
        16-byte aligned, a layer's query / key / value copies adjacent; _Linear takes the views as they lie, so a
        forward casts no matrix.  The results are bit-identical to the per-forward casts.  The copies follow the masters
        through the optimizer step and load_state_dict; after any other edit of a master call refresh_half_weights()."""
        if self._half is None or self._half.moved():
            groups = (linear_groups("bert_q", self.config, "proj_q") + linear_groups("bert_c", self.config, "proj_c"))
            self._half = HalfWeights(self._flat, groups)
        else:
            self._half.refresh()
        return dict(self._half.copies)

    def refresh_half_weights(self):
        """Cast every master matrix into its working copy again (one launch); nothing to do without half_weights()."""
        if self._half is not None:
            self._half.refresh()

    def dropout_state(self):
        """(seed, call): what, with the rates, determines every mask of the next tower pass; `call` advances once per
        tower pass in train() mode with a rate above 0 (24 bits, wraps).  Save it next to a checkpoint to resume."""
        return self._dropout_seed, self._dropout_call

    def set_dropout_state(self, state):
        seed, call = state
        self._dropout_seed, self._dropout_call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFF

    def _apply(self, fn, *args, **kwargs):
        probe = fn(torch.empty(0, dtype=torch.float32, device=self.device))
        if probe.device.type != "cuda":
            raise RuntimeError("proqa_amd.TrainableRetriever runs on MI355X only; there is no CPU path")
        if probe.dtype != torch.float32:
            raise RuntimeError("the parameters are the fp32 masters; the module casts them to fp16 itself")
        if probe.device != self.device:
            self.device = probe.device
        result = super()._apply(fn, *args, **kwargs)
        if self._half is not None:
            if self._half.moved():
                self._half = None        # the copies belong to storage that is gone: back to the per-forward casts
            else:
                self._half.refresh()     # fn may have edited the masters in place
        return result

    # -- forward ----------------------------------------------------------------------------
    def forward(self, batch):
        """batch: one re_collate batch -> {'q', 'c'}; or a LIST of them (the micro-batches of one accumulation window, whose
        weights are the same) -> {'q', 'c', 'block_sizes'}: ONE pass per tower over all rows, rows in the list's order,
        block_sizes the rows of every batch (what inbatch_loss_blocks takes).  Batches of different widths are right-padded
        to the widest on the device: run_tower packs the tokens by cu_seqlens, so the padding costs nothing further.
        Dropout takes one (seed, call) per tower pass, as for a single batch."""
        if isinstance(batch, (list, tuple)):
            if not batch:
                raise ValueError("TrainableRetriever.forward: an empty list of batches")
            sizes = [b["input_ids_q"].shape[0] for b in batch]
            if any(b["input_ids_c"].shape[0] != n or n < 1 for b, n in zip(batch, sizes)):
                raise ValueError("TrainableRetriever.forward: every batch of a list needs as many paragraphs as questions (>= 1)")
            out = self.forward({k: _cat_right_padded([b[k] for b in batch])
                                for k in ("input_ids_q", "input_mask_q", "input_ids_c", "input_mask_c")})
            out["block_sizes"] = sizes
            return out
        return {"q": self._tower("bert_q", "proj_q", batch["input_ids_q"], batch["input_mask_q"]),
                "c": self._tower("bert_c", "proj_c", batch["input_ids_c"], batch["input_mask_c"])}

    def get_embed(self, batch, is_query_embed, check_mask=True, seq_lens_host=None):
        """The reference's get_embed (retriever.py:33-43); call it under torch.no_grad() for evaluation.  With
        check_mask=False and seq_lens_host (the rows' lengths, as BertForRetriever.get_embed takes them) the pass does not
        read the mask and makes no host round trip."""
        tower, proj = ("bert_q", "proj_q") if is_query_embed else ("bert_c", "proj_c")
        if check_mask and seq_lens_host is not None:
            seq_lens_host = None        # the mask is checked: its own lengths are used
        return {"embed": self._tower(tower, proj, batch["input_ids"], batch["input_mask"], seq_lens_host)}

    def _tower(self, tower, proj, input_ids, input_mask, seq_lens_host=None):
        if not input_ids.is_cuda:
            raise RuntimeError("TrainableRetriever expects CUDA tensors (the reference feeds move_to_cuda(batch))")
        if input_ids.shape[0] == 0:
            return torch.empty((0, EMBED_DIM), dtype=torch.float16, device=self.device)
        # dropout: one `call` per tower pass, so the two towers of a step differ
        p_hid = self.hidden_dropout_prob if self.training else 0.0
        p_att = self.attention_probs_dropout_prob if self.training else 0.0
        seed, call = self._dropout_seed, self._dropout_call
        if p_hid > 0 or p_att > 0:
            self._dropout_call = (call + 1) & 0xFFFFFF
        return run_tower(self._flat, tower, self.config, input_ids, input_mask, proj=proj, drop=(p_hid, p_att, seed, call),
                         half=self._half.views if self._half is not None else None, seq_lens_host=seq_lens_host,
                         deterministic=self.deterministic)
