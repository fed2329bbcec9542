"""In-batch scoring of a collated batch of (question, paragraph) embeddings on the GPU.

Replaces `product = torch.mm(q, c.t()); product.argmax(-1) == target; CrossEntropyLoss(product, target)` of
/root/reference/retrieval/train_retriever.py:203-205 and :313-318 by one call of proqa_inbatch_eval_f16: the
[nq, nc] product is never formed.  Everything stays on the device and on torch's current stream; only
inbatch_accuracy_and_loss copies two numbers to the host.
"""
import torch

from . import _lib
from ._lib import EMBED_DIM


def _rows_f16(x, name):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"inbatch_eval: {name} must be a CUDA tensor")
    if x.dim() != 2:
        raise ValueError(f"inbatch_eval: {name} must be [n, {EMBED_DIM}], got {tuple(x.shape)}")
    if x.dtype != torch.float16:
        # the towers emit fp16 (model.half()); rounding other types here would be silent, checking them a host sync
        raise ValueError(f"inbatch_eval: {name} must be float16, got {x.dtype}")
    return x.contiguous()


def inbatch_eval(q, c, target=None):
    """q [nq, 128], c [nc, 128] fp16 device tensors, target int [nq] (None: target[i] = i, needs nq <= nc) ->
    {'argmax': int32 [nq], 'rank': int32 [nq], 'max': float32 [nq], 'gold': float32 [nq], 'lse': float32 [nq]}, all on
    the device (see proqa_hip.h for the tie and non-finite rules).  No synchronisation."""
    lib = _lib.load()
    q, c = _rows_f16(q, "q"), _rows_f16(c, "c")
    if q.device != c.device:
        raise ValueError("inbatch_eval: q and c live on different devices")
    nq, nc = q.shape[0], c.shape[0]
    dim = q.shape[1]
    if c.shape[1] != dim:
        raise ValueError(f"inbatch_eval: q is [{nq}, {dim}] but c is [{nc}, {c.shape[1]}]")
    t = None
    if target is not None:
        if target.shape != (nq,):
            raise ValueError(f"inbatch_eval: target must be [{nq}], got {tuple(target.shape)}")
        t = target.to(device=q.device, dtype=torch.int32).contiguous()
    dev = q.device
    out = {"argmax": torch.empty(nq, dtype=torch.int32, device=dev), "rank": torch.empty(nq, dtype=torch.int32, device=dev),
           "max": torch.empty(nq, dtype=torch.float32, device=dev), "gold": torch.empty(nq, dtype=torch.float32, device=dev),
           "lse": torch.empty(nq, dtype=torch.float32, device=dev)}
    with torch.cuda.device(dev):
        _lib.check(lib.proqa_inbatch_eval_f16(q.data_ptr(), c.data_ptr(), t.data_ptr() if t is not None else None, nq, nc, dim,
                                              out["argmax"].data_ptr(), out["rank"].data_ptr(), out["max"].data_ptr(),
                                              out["gold"].data_ptr(), out["lse"].data_ptr(), _lib.current_stream_ptr()))
    return out


MAX_BLOCKS = 64      # PROQA_INBATCH_MAX_BLOCKS


def block_offsets(block_sizes, n):
    """block_sizes (M ints >= 1 that sum to n, or an int tensor on the host) -> the host int32 [M + 1] offsets the block
    entry points take (a ctypes array; the library copies them into the kernel arguments during the call)."""
    import ctypes
    sizes = [int(b) for b in (block_sizes.tolist() if torch.is_tensor(block_sizes) else block_sizes)]
    if not 1 <= len(sizes) <= MAX_BLOCKS:
        raise ValueError(f"inbatch blocks: {len(sizes)} blocks, must be in [1, {MAX_BLOCKS}]")
    if any(b < 1 for b in sizes) or sum(sizes) != n:
        raise ValueError(f"inbatch blocks: block_sizes {sizes} must be positive and sum to the {n} rows")
    offsets = (ctypes.c_int32 * (len(sizes) + 1))()
    for m, b in enumerate(sizes):
        offsets[m + 1] = offsets[m] + b
    return offsets


def inbatch_eval_blocks(q, c, offsets):
    """The block-diagonal objective's forward (proqa_inbatch_loss_blocks_f16): q, c [n, 128] fp16 device tensors, offsets
    from block_offsets() -> {'lse': float32 [n], 'gold': float32 [n], 'loss': float32 [M]} on the device: per row the
    log-sum-exp over its OWN block's columns and the diagonal score, per block mean(lse - gold).  No synchronisation."""
    lib = _lib.load()
    q, c = _rows_f16(q, "q"), _rows_f16(c, "c")
    if q.device != c.device or q.shape != c.shape:
        raise ValueError(f"inbatch_eval_blocks: q {tuple(q.shape)} on {q.device} and c {tuple(c.shape)} on {c.device} must match")
    n, dim, M = q.shape[0], q.shape[1], len(offsets) - 1
    dev = q.device
    out = {"lse": torch.empty(n, dtype=torch.float32, device=dev), "gold": torch.empty(n, dtype=torch.float32, device=dev),
           "loss": torch.empty(M, dtype=torch.float32, device=dev)}
    with torch.cuda.device(dev):
        _lib.check(lib.proqa_inbatch_loss_blocks_f16(q.data_ptr(), c.data_ptr(), offsets, M, n, dim, out["lse"].data_ptr(),
                                                     out["gold"].data_ptr(), out["loss"].data_ptr(),
                                                     _lib.current_stream_ptr()))
    return out


def inbatch_accuracy_and_loss(q, c, target=None):
    """(num_correct, sum over the rows of lse - gold) of one batch as Python numbers: ONE host copy.  num_correct counts
    the rows whose argmax is their target (the reference's `prediction == target`); the second is the batch's
    CrossEntropyLoss times its size."""
    out = inbatch_eval(q, c, target)
    nq = q.shape[0]
    if nq == 0:
        return 0, 0.0
    t = torch.arange(nq, device=out["argmax"].device, dtype=torch.int32) if target is None else \
        target.to(device=out["argmax"].device, dtype=torch.int32)
    both = torch.stack([(out["argmax"] == t).sum().to(torch.float64), (out["lse"] - out["gold"]).sum(dtype=torch.float64)]).cpu()
    return int(both[0]), float(both[1])
