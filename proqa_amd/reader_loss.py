"""The reader's training objective on MI355X: span + rank loss of one question's passages, with gradients.

Replaces qa/bert_retrieve_qa.py:64-171 of the reference as qa/train_dense_qa.sh trains it (--shared-norm, joint loss,
early loss over the sampler's top-5000): the qa_outputs head, the paragraph mask, both normalisations, the rank softmax
over para_embed and the marginal over the answer positions are proqa_reader_loss_f16 (three launches), the gradient is
proqa_reader_loss_backward_f16 (four launches).  No Python loop, no nonzero(), no device-to-host copy, and the [T, 2]
logit gradient is never stored: it lives in fp32 registers, so a loss scale of 2^16 does not overflow it.

reader_loss_multi is the same objective over the passages of Q questions in ONE call (proqa_reader_loss_multi_f16: the
same seven kernels with a question dimension); each question's values carry the bits reader_loss gives for it alone.

torch computes nothing here: it owns the memory and the stream, casts the fp32 masters to fp16 (as trainable.py does) and
the sampler's int64 positions / labels to the int32 the kernels take, and autograd carries the four gradients.
"""
import numpy as np
import torch

from . import _lib
from ._lib import EMBED_DIM
from .trainable import _workspace

SHARED_NORM = 1
NO_EARLY = 2
READER_HEAD_SITE = 255     # the dropout site reserved for the reader head (csrc/dropout_rng.h)
MAX_SEQ_LEN = 4096


def _i32(x, device, name):
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    if x.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"reader_loss: {name} must be an integer tensor, got {x.dtype}")
    return x.to(device=device, dtype=torch.int32).contiguous()


class _Geometry:
    """What both kernels are told about the batch (plain numbers and the int32 device tensors).  Without question_seq: one
    question, in the packed or the padded layout.  With question_seq / question_para (the CSR offsets that cut the batch into
    n_questions: host lists, or int device tensors together with max_seqs / max_paras): a pack, in the packed layout."""

    def __init__(self, hidden, cu_seqlens, seq_lens, para_offset, start_positions, end_positions, para_embed, labels,
                 shared_norm, early, qa_drop, dropout_state, max_seq_len, n_questions=1, question_seq=None, question_para=None,
                 max_seqs=None, max_paras=None):
        dev = hidden.device
        if (cu_seqlens is None) == (seq_lens is None):
            raise ValueError("reader_loss: exactly one of cu_seqlens (packed hidden [T, H]) and seq_lens (padded hidden "
                             "[B, L, H]) must be given")
        if cu_seqlens is not None:
            if hidden.dim() != 2:
                raise ValueError(f"reader_loss: packed hidden must be [T, H], got {tuple(hidden.shape)}")
            self.cu, self.lens = _i32(cu_seqlens, dev, "cu_seqlens"), None
            self.batch = self.cu.numel() - 1
            self.seq_len = int(max_seq_len) if max_seq_len is not None else min(max(hidden.shape[0], 1), MAX_SEQ_LEN)
        else:
            if hidden.dim() != 3:
                raise ValueError(f"reader_loss: padded hidden must be [B, L, H], got {tuple(hidden.shape)}")
            self.cu, self.lens = None, _i32(seq_lens, dev, "seq_lens")
            self.batch, self.seq_len = hidden.shape[0], hidden.shape[1]
            if self.lens.numel() != self.batch:
                raise ValueError(f"reader_loss: seq_lens must be [{self.batch}]")
        self.hidden_size = hidden.shape[-1]
        self.para_offset = _i32(para_offset, dev, "para_offset")
        self.start, self.end = _i32(start_positions, dev, "start_positions"), _i32(end_positions, dev, "end_positions")
        if self.start.dim() != 2 or self.start.shape != self.end.shape or self.start.shape[0] != self.batch:
            raise ValueError(f"reader_loss: start / end positions must both be [{self.batch}, A], got "
                             f"{tuple(self.start.shape)} and {tuple(self.end.shape)}")
        if self.para_offset.numel() != self.batch:
            raise ValueError(f"reader_loss: para_offset must be [{self.batch}]")
        self.n_answers = self.start.shape[1]
        if not para_embed.is_cuda or para_embed.dim() != 2 or para_embed.dtype not in (torch.float16, torch.float32):
            raise ValueError("reader_loss: para_embed must be a float16 or float32 [P, 128] CUDA tensor")
        self.para = para_embed.contiguous()
        self.para_dtype = _lib.PROQA_F16 if para_embed.dtype == torch.float16 else _lib.PROQA_F32
        self.n_paras, self.dim = para_embed.shape
        self.labels = _i32(labels, dev, "top5000_labels").reshape(-1)
        if self.labels.numel() != self.n_paras:
            raise ValueError(f"reader_loss: top5000_labels must be [{self.n_paras}], got {self.labels.numel()}")
        self.flags = (SHARED_NORM if shared_norm else 0) | (0 if early else NO_EARLY)
        self.p = float(qa_drop)
        if self.p > 0:
            if dropout_state is None:
                raise ValueError("reader_loss: qa_drop > 0 needs dropout_state=(seed, call)")
            seed, call = dropout_state
            self.seed, self.call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFF
        else:
            self.seed, self.call = 0, 0
        self.pack = question_seq is not None
        self.n_questions = int(n_questions) if self.pack else 1
        self.per_question = (self.n_questions,) if self.pack else ()     # the leading shape of loss_out and d_q
        if not self.pack:
            return
        self.host = []
        counts = []
        for name, csr, given in (("question_seq", question_seq, max_seqs), ("question_para", question_para, max_paras)):
            if torch.is_tensor(csr):
                if given is None:
                    raise ValueError(f"reader_loss_multi: {name} on the device needs max_seqs= and max_paras= (the largest "
                                     "per-question counts); a host list carries them itself")
                self.host.append(None)
                counts.append(int(given))
            else:
                arr = np.ascontiguousarray(np.asarray(list(csr), dtype=np.int64).astype(np.int32))
                if arr.ndim != 1 or arr.size < 2:
                    raise ValueError(f"reader_loss_multi: {name} must hold n_questions + 1 offsets")
                self.host.append(arr)
                counts.append(int(np.diff(arr).max()) if given is None else int(given))
                csr = torch.from_numpy(arr).pin_memory().to(dev, non_blocking=True)     # (an upload the host does not wait for)
            csr = _i32(csr, dev, name).reshape(-1)
            if csr.numel() != self.n_questions + 1:
                raise ValueError(f"reader_loss_multi: {name} must be [{self.n_questions + 1}] for q [{self.n_questions}, "
                                 f"{EMBED_DIM}], got {csr.numel()}")
            setattr(self, name, csr)
        if (self.host[0] is None) != (self.host[1] is None):
            raise ValueError("reader_loss_multi: question_seq and question_para must both be host lists or both be tensors")
        self.max_seqs, self.max_paras = counts

    def layout(self):
        """the arguments between hidden and qa_w (a pack has no seq_lens)"""
        lens = () if self.pack else (self.lens.data_ptr() if self.lens is not None else None,)
        return (*lens, self.cu.data_ptr() if self.cu is not None else None, self.batch, self.seq_len, self.hidden_size,
                self.para_offset.data_ptr())

    def objective(self, q):
        """the arguments from start_pos to call (a pack puts its questions between dim and flags)"""
        questions = ()
        if self.pack:
            host = [a.ctypes.data if a is not None else None for a in self.host]
            questions = (self.question_seq.data_ptr(), self.question_para.data_ptr(), self.n_questions, self.max_seqs,
                         self.max_paras, host[0], host[1])
        return (self.start.data_ptr(), self.end.data_ptr(), self.n_answers, q.data_ptr(), self.para.data_ptr(), self.para_dtype,
                self.labels.data_ptr(), self.n_paras, self.dim, *questions, self.flags, self.p, self.seed, READER_HEAD_SITE,
                self.call)

    def entries(self, lib):
        """(forward, backward) of the C ABI: a pack takes the multi pair, at one question too"""
        if self.pack:
            return lib.proqa_reader_loss_multi_f16, lib.proqa_reader_loss_multi_backward_f16
        return lib.proqa_reader_loss_f16, lib.proqa_reader_loss_backward_f16

    def workspace(self, lib, device):
        if self.pack:
            need = lib.proqa_reader_loss_multi_workspace_bytes(self.n_questions, self.batch, self.seq_len, self.hidden_size,
                                                               self.n_answers, self.n_paras, self.max_paras)
        else:
            need = lib.proqa_reader_loss_workspace_bytes(self.batch, self.seq_len, self.hidden_size, self.n_answers, self.n_paras)
        return _workspace(device, need)


def reader_loss_forward(hidden, w16, b16, q, geo):
    """-> (loss_out fp32 [3] = total, joint, early, for a pack [Q, 3]; logits fp16 [rows, 2]; stats fp32 [8 Q + 2 B], the
    single-question layout question after question); no autograd"""
    lib = _lib.load()
    dev = hidden.device
    rows = hidden.numel() // max(geo.hidden_size, 1)
    logits = torch.empty((rows, 2), dtype=torch.float16, device=dev)
    stats = torch.empty(8 * geo.n_questions + 2 * max(geo.batch, 0), dtype=torch.float32, device=dev)
    loss_out = torch.empty(geo.per_question + (3,), dtype=torch.float32, device=dev)
    ws = geo.workspace(lib, dev)
    with torch.cuda.device(dev):
        _lib.check(geo.entries(lib)[0](hidden.data_ptr(), *geo.layout(), w16.data_ptr(), b16.data_ptr(), *geo.objective(q),
                                       logits.data_ptr(), stats.data_ptr(), loss_out.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _lib.current_stream_ptr()))
    return loss_out, logits, stats


def reader_loss_backward(hidden, w16, q, geo, logits, stats, grad_in):
    """grad_in: fp32 on the device, one value per question -> (d_hidden fp16 like hidden, d_qa_w fp32 [2, H], d_qa_b fp32 [2],
    d_q fp16 [128], for a pack [Q, 128])"""
    lib = _lib.load()
    dev = hidden.device
    d_hidden = torch.empty_like(hidden)
    d_w = torch.empty((2, geo.hidden_size), dtype=torch.float32, device=dev)
    d_b = torch.empty(2, dtype=torch.float32, device=dev)
    d_q = torch.empty(geo.per_question + (EMBED_DIM,), dtype=torch.float16, device=dev)
    ws = geo.workspace(lib, dev)
    with torch.cuda.device(dev):
        _lib.check(geo.entries(lib)[1](hidden.data_ptr(), *geo.layout(), w16.data_ptr(), *geo.objective(q), logits.data_ptr(),
                                       stats.data_ptr(), grad_in.data_ptr(), d_hidden.data_ptr(), d_w.data_ptr(), d_b.data_ptr(),
                                       d_q.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()))
    return d_hidden, d_w, d_b, d_q


# the names and the argument order under which tests/test_reader_loss_multi_gpu.py drives a pack through the helpers
reader_loss_multi_forward, reader_loss_multi_backward = reader_loss_forward, reader_loss_backward


def _MultiGeometry(hidden, n_questions, cu_seqlens, question_seq, question_para, max_seqs, max_paras, *rest):
    return _Geometry(hidden, cu_seqlens, None, *rest, n_questions=n_questions, question_seq=question_seq,
                     question_para=question_para, max_seqs=max_seqs, max_paras=max_paras)


class _ReaderLoss(torch.autograd.Function):
    """(hidden fp16, qa_weight fp32 master, qa_bias fp32 master, q fp16 [128] or, for a pack, [Q, 128]) -> fp32 [3] or [Q, 3]
    = (loss, joint, early) per question; only element 0 of a question is differentiated."""

    @staticmethod
    def forward(ctx, hidden, qa_weight, qa_bias, q, geo):
        w16, b16 = qa_weight.half().contiguous(), qa_bias.half().contiguous()
        loss_out, logits, stats = reader_loss_forward(hidden, w16, b16, q, geo)
        ctx.save_for_backward(hidden, w16, q, logits, stats)
        ctx.geo = geo
        return loss_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        hidden, w16, q, logits, stats = ctx.saved_tensors
        g = grad_out[..., 0].to(torch.float32).contiguous()     # the gradients of the questions' total losses
        d_hidden, d_w, d_b, d_q = reader_loss_backward(hidden, w16, q, ctx.geo, logits, stats, g)
        return d_hidden, d_w, d_b, d_q, None


def _check_arguments(who, hidden, qa_weight, qa_bias, q, q_dims_ok, q_shape, qa_drop):
    """what both fronts refuse before anything is built; q_dims_ok / q_shape: the front's own rule for q's dimensions"""
    if not torch.is_tensor(hidden) or not hidden.is_cuda or hidden.dtype != torch.float16:
        raise ValueError(f"{who}: hidden must be a float16 CUDA tensor (there is no CPU path)")
    if not q.is_cuda or q.dtype != torch.float16 or not q_dims_ok or q.shape[-1] != EMBED_DIM:
        raise ValueError(f"{who}: q must be a float16 CUDA tensor {q_shape}, got {q.dtype} {tuple(q.shape)}")
    if qa_weight.dtype != torch.float32 or qa_bias.dtype != torch.float32:
        raise ValueError(f"{who}: qa_weight / qa_bias are the fp32 masters; they are cast to fp16 inside")
    if tuple(qa_weight.shape) != (2, hidden.shape[-1]) or tuple(qa_bias.shape) != (2,):
        raise ValueError(f"{who}: qa_weight must be [2, {hidden.shape[-1]}] and qa_bias [2]")
    if not 0.0 <= float(qa_drop) <= 0.9:
        raise ValueError(f"{who}: qa_drop={qa_drop!r} must be in [0, 0.9]")


def reader_loss(hidden, qa_weight, qa_bias, q, para_embed, top5000_labels, start_positions, end_positions, para_offset, *,
                cu_seqlens=None, seq_lens=None, shared_norm=True, early=True, qa_drop=0.0, dropout_state=None,
                max_seq_len=None):
    """The training loss of BertRetrieveQA.forward for the B passages of one question.

    hidden            fp16 last hidden state of the reader's BERT: packed [T, H] with cu_seqlens (int [B + 1]), or padded
                      [B, L, H] with seq_lens (int [B]); H % 8 == 0, H <= 1024
    qa_weight/qa_bias the fp32 masters of qa_outputs, [2, H] and [2]; their gradients are fp32
    q                 fp16 question embedding [128], or [n, 128] of which row 0 is taken (the reference's q[0]), e.g.
                      TrainableRetriever.get_embed(batch, True)["embed"]
    para_embed        [P, 128] float16 or float32, the sampler's rows; the first B belong to the sequences
    top5000_labels    int [P]; start_positions / end_positions: int [B, A] in sequence coordinates, -1 = padding
    para_offset       int [B]: the paragraph mask of sequence b is [para_offset[b], len(b) - 1)
    shared_norm       --shared-norm; early=False is --drop-early (the loss without the early term)
    qa_drop           rate of the dropout in front of qa_outputs; dropout_state = (seed, call), call advanced by the caller
    max_seq_len       packed layout only: a bound on the longest sequence (default min(T, 4096))

    -> {"loss": fp32 scalar with gradients w.r.t. hidden, q, qa_weight and qa_bias, "joint", "early": fp32 scalars, detached}.
    Everything stays on the device and on torch's current stream."""
    _check_arguments("reader_loss", hidden, qa_weight, qa_bias, q, q.dim() in (1, 2), f"[{EMBED_DIM}] or [n, {EMBED_DIM}]",
                     qa_drop)
    geo = _Geometry(hidden.contiguous(), cu_seqlens, seq_lens, para_offset, start_positions, end_positions, para_embed,
                    top5000_labels, shared_norm, early, qa_drop, dropout_state, max_seq_len)
    q0 = (q[0] if q.dim() == 2 else q).contiguous()
    out = _ReaderLoss.apply(hidden.contiguous(), qa_weight, qa_bias, q0, geo)
    return {"loss": out[0], "joint": out[1].detach(), "early": out[2].detach()}


def reader_loss_multi(hidden, qa_weight, qa_bias, q, para_embed, top5000_labels, start_positions, end_positions, para_offset, *,
                      cu_seqlens, question_seq, question_para, shared_norm=True, early=True, qa_drop=0.0, dropout_state=None,
                      max_seq_len=None, max_seqs=None, max_paras=None):
    """reader_loss for the passages of Q questions in one call (proqa_reader_loss_multi_f16): one autograd node, three
    launches forward and four backward whatever Q is, no host wait.

    hidden            packed fp16 [T, H] with cu_seqlens (int [B + 1]) over the sequences of ALL questions, question after
                      question; start_positions / end_positions [B, A] and para_offset [B] likewise
    q                 fp16 [Q, 128], one question embedding per question
    para_embed        [P, 128] float16 or float32 and top5000_labels [P]: every question's rows, question after question; the
                      first B_i rows of question i belong to its sequences
    question_seq      [Q + 1] offsets into the sequences, question_para [Q + 1] offsets into the rows of para_embed: host
                      lists (they are checked, and uploaded with the other integer tensors) or int device tensors (then
                      max_seqs / max_paras, the largest per-question counts, must be given and nothing can be checked: the
                      kernels clamp)
    qa_weight, qa_bias, shared_norm, early, qa_drop, dropout_state, max_seq_len: as reader_loss, one value for the call.  With
    qa_drop > 0 the mask coordinate is the packed row of the whole pack.

    -> {"losses": fp32 [Q] with gradients w.r.t. hidden, q, qa_weight and qa_bias, "joint", "early": fp32 [Q], detached}.
    Each question's values carry the bits reader_loss gives for the question alone (qa_drop == 0); the gradients of qa_weight /
    qa_bias are the questions' gradients added in ascending order."""
    _check_arguments("reader_loss_multi", hidden, qa_weight, qa_bias, q, q.dim() == 2 and q.shape[0] >= 1,
                     f"[Q, {EMBED_DIM}] with Q >= 1", qa_drop)
    if cu_seqlens is None:
        raise ValueError("reader_loss_multi: the packed layout only (cu_seqlens)")
    geo = _Geometry(hidden.contiguous(), cu_seqlens, None, para_offset, start_positions, end_positions, para_embed,
                    top5000_labels, shared_norm, early, qa_drop, dropout_state, max_seq_len, n_questions=q.shape[0],
                    question_seq=question_seq, question_para=question_para, max_seqs=max_seqs, max_paras=max_paras)
    out = _ReaderLoss.apply(hidden.contiguous(), qa_weight, qa_bias, q.contiguous(), geo)
    return {"losses": out[:, 0], "joint": out[:, 1].detach(), "early": out[:, 2].detach()}
