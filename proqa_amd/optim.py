"""FusedAdamW: the optimizer step of retriever training on libproqa_hip.so's fused kernels.

What the reference's loop runs between `loss.backward()` and the next forward (retrieval/train_retriever.py:207-214: apex
amp's unscale and overflow check, `clip_grad_norm_`, `transformers.AdamW.step`) is three launches here
(include/proqa_hip.h, proqa_adamw_step): partial sums of squares of the unscaled gradients, one workgroup that turns them
into the norm, the skip decision, the clip coefficient, the bias corrections and the next loss scale, and one pass that
reads g, p, m, v and writes p, m, v.  `step()` never copies from the device and never waits for it: the step count, the
loss scale and the last norm live in device memory and are handed out as tensors.

    opt = FusedAdamW(groups, lr=1e-5, max_grad_norm=2.0, loss_scale="dynamic")
    opt.scale_loss(loss).backward(); opt.step(); scheduler.step(); opt.zero_grad()

Semantics.  The default is the reference's optimizer, `transformers.AdamW(correct_bias=True)`: eps is added to sqrt(v)
BEFORE the bias correction and the decoupled weight decay is applied AFTER the Adam update.  `torch_semantics=True` is
`torch.optim.AdamW` (eps after the bias correction, decay first) for users who trained with that class.

Deviation from both: there is ONE step count for the whole optimizer, not one per parameter.  They differ only for a
parameter that had no gradient in some step; such a parameter is skipped (p, exp_avg, exp_avg_sq untouched), as
`if p.grad is None: continue` does, but its bias correction follows the global count.
"""
import ctypes

import numpy as np
import torch

from . import _lib

# numpy mirror of proqa_adamw_tensor
_TENSOR_DTYPE = np.dtype([("p", np.uint64), ("g", np.uint64), ("m", np.uint64), ("v", np.uint64), ("n", np.int64),
                          ("lr", np.float64), ("weight_decay", np.float64)])
assert _TENSOR_DTYPE.itemsize == ctypes.sizeof(_lib.AdamwTensor)

DYNAMIC_INIT_SCALE = 65536.0     # apex amp's dynamic scaler starts at 2**16


def _chunk_map(lib, sizes):
    """(device-ready int32 [n_chunks, 2] array, n_chunks) of proqa_adamw_chunk_map for these tensor sizes"""
    n = len(sizes)
    n_chunks = lib.proqa_adamw_chunk_map(sizes.ctypes.data, n, None, 0)
    if n_chunks < 0:
        _lib.check(int(n_chunks))
    chunks = np.zeros((max(int(n_chunks), 1), 2), dtype=np.int32)
    if lib.proqa_adamw_chunk_map(sizes.ctypes.data, n, chunks.ctypes.data, n_chunks) != n_chunks:
        _lib.check(-1)
    return chunks, int(n_chunks)


def cast_half_tensors(masters, copies):
    """copies[i][...] = masters[i].to(float16) for contiguous fp32 CUDA masters and contiguous fp16 copies of the same
    numel on one device (None: no copy): one launch of proqa_cast_half_tensors, no host wait.  The tables are built and
    uploaded per call: this is for construction and for re-casts after an edit, not for the training step."""
    lib = _lib.load()
    _lib.require_gpu()
    if len(masters) != len(copies) or not masters:
        raise ValueError("cast_half_tensors takes as many copies as masters, at least one")
    dev = masters[0].device
    for p, h in zip(masters, copies):
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
            raise ValueError("cast_half_tensors takes contiguous fp32 CUDA masters of one device")
        if h is not None and (h.dtype != torch.float16 or not h.is_contiguous() or h.device != dev or h.numel() != p.numel()):
            raise ValueError("a half copy must be a contiguous float16 tensor of its master's numel and device")
    table = np.zeros(len(masters), dtype=_TENSOR_DTYPE)
    table["p"] = [p.data_ptr() for p in masters]
    table["n"] = [p.numel() for p in masters]
    chunks, n_chunks = _chunk_map(lib, np.ascontiguousarray(table["n"]))
    ptrs = np.array([0 if h is None else h.data_ptr() for h in copies], dtype=np.uint64)
    with torch.cuda.device(dev):
        table_dev = torch.from_numpy(table.view(np.uint8)).to(dev)
        chunks_dev = torch.from_numpy(chunks).to(dev)
        ptrs_dev = torch.from_numpy(ptrs.view(np.int64)).to(dev)
        _lib.check(lib.proqa_cast_half_tensors(table_dev.data_ptr(), ptrs_dev.data_ptr(), len(masters), chunks_dev.data_ptr(),
                                               n_chunks, _lib.current_stream_ptr()))
        for t in (table_dev, chunks_dev, ptrs_dev):      # the launch reads them on this stream: no reuse before it ran
            t.record_stream(torch.cuda.current_stream())


class FusedAdamW(torch.optim.Optimizer):
    """AdamW over fp32 CUDA parameters, one fused step for all of them.

    max_grad_norm: clip the global gradient norm (torch.nn.utils.clip_grad_norm_'s rule), None = no clipping.
    loss_scale: None (gradients are not scaled), a float (fixed scale) or "dynamic" (apex amp O1's scaler: starts at
        2**16, halves on an overflowing step, which is skipped, doubles after growth_interval clean steps).
    With both None the class is a plain optimizer (one launch per step) that also works under torch.amp.GradScaler.

    `betas` and `eps` hold for the whole optimizer; `lr` and `weight_decay` are per group and read at every step, so
    schedulers that edit param_groups[i]["lr"] work.  Gradients may be reallocated, left None or accumulated over several
    backward() calls between steps.

    half_copies: {parameter: fp16 tensor} (TrainableRetriever.half_weights() returns one).  The step that writes a
    parameter writes its fp16 working copy in the same pass (proqa_adamw_step_half), so that no forward has to cast the
    master again.  A copy has the parameter's numel, is contiguous fp16 on its device; the optimizer keeps it alive.  A
    skipped step and a parameter without a gradient leave p, and therefore the copy, as they are."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, loss_scale=None,
                 growth_interval=2000, torch_semantics=False, backoff_factor=0.5, growth_factor=2.0, half_copies=None):
        if not lr >= 0.0:
            raise ValueError(f"invalid learning rate: {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"betas {betas} must lie in [0, 1)")
        if not eps >= 0.0:
            raise ValueError(f"invalid eps: {eps}")
        if not weight_decay >= 0.0:
            raise ValueError(f"invalid weight_decay: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"max_grad_norm must be positive or None, not {max_grad_norm}")
        if loss_scale is None:
            self._scale_mode, init_scale = _lib.ADAMW_SCALE_NONE, 1.0
        elif loss_scale == "dynamic":
            self._scale_mode, init_scale = _lib.ADAMW_SCALE_DYNAMIC, DYNAMIC_INIT_SCALE
        elif isinstance(loss_scale, (int, float)) and not isinstance(loss_scale, bool):
            if not (loss_scale > 0.0 and loss_scale < float("inf")):
                raise ValueError(f"loss_scale must be positive and finite, not {loss_scale}")
            self._scale_mode, init_scale = _lib.ADAMW_SCALE_FIXED, float(loss_scale)
        else:
            raise ValueError(f"loss_scale must be None, a number or 'dynamic', not {loss_scale!r}")
        if int(growth_interval) < 1:
            raise ValueError("growth_interval must be at least 1")
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay))
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.torch_semantics = bool(torch_semantics)
        self.growth_interval = int(growth_interval)
        self.backoff_factor, self.growth_factor = float(backoff_factor), float(growth_factor)
        self._plain = self.max_grad_norm is None and self._scale_mode == _lib.ADAMW_SCALE_NONE
        self._plain_step = 0

        self._params = [p for group in self.param_groups for p in group["params"]]
        if not self._params:
            raise ValueError("FusedAdamW got no parameters")
        for p in self._params:
            if not p.is_cuda or p.dtype != torch.float32 or p.is_sparse or not p.is_contiguous():
                raise ValueError("FusedAdamW takes contiguous fp32 CUDA parameters; got "
                                 f"{p.dtype} on {p.device}{'' if p.is_contiguous() else ', not contiguous'}")
            if p.device != self._params[0].device:
                raise ValueError("FusedAdamW takes parameters of one device")
        self._device = self._params[0].device
        self._half = self._check_half_copies(half_copies)
        self._lib = _lib.load()
        _lib.require_gpu()
        for p in self._params:
            self.state[p] = {"exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                             "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}

        # the chunk map depends on the sizes only: built and uploaded once
        n = len(self._params)
        sizes = np.array([p.numel() for p in self._params], dtype=np.int64)
        chunks, self._n_chunks = _chunk_map(self._lib, sizes)
        self._chunks_dev = torch.from_numpy(chunks).to(self._device)
        self._table = np.zeros(n, dtype=_TENSOR_DTYPE)
        self._table["n"] = sizes
        self._table_dev = torch.empty(self._table.nbytes, dtype=torch.uint8, device=self._device)
        ws_bytes = int(self._lib.proqa_adamw_workspace_bytes(self._n_chunks))
        self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self._device)
        self._state_dev = torch.zeros(_lib.ADAMW_STATE_BYTES, dtype=torch.uint8, device=self._device)
        self._refresh_static_pointers()
        # the copies never move: their pointer array is uploaded once
        self._half_dev = None
        if self._half is not None:
            ptrs = np.array([0 if h is None else h.data_ptr() for h in self._half], dtype=np.uint64)
            self._half_dev = torch.from_numpy(ptrs.view(np.int64)).to(self._device)
        self._init_device_state(0, init_scale, 0, 0)

    def _check_half_copies(self, half_copies):
        if half_copies is None:
            return None
        if not hasattr(half_copies, "items"):
            raise ValueError("half_copies must be a {parameter: fp16 tensor} mapping")
        by_id = {id(p): i for i, p in enumerate(self._params)}
        copies = [None] * len(self._params)
        for p, h in half_copies.items():
            if id(p) not in by_id:
                raise ValueError("half_copies names a tensor that is not a parameter of this optimizer")
            if not isinstance(h, torch.Tensor) or h.dtype != torch.float16:
                raise ValueError(f"a half copy must be a float16 tensor, got {getattr(h, 'dtype', type(h))}")
            if h.numel() != p.numel():
                raise ValueError(f"a half copy must have its parameter's {p.numel()} elements, got {h.numel()}")
            if h.device != p.device:
                raise ValueError(f"a half copy must live on its parameter's device {p.device}, got {h.device}")
            if not h.is_contiguous():
                raise ValueError("a half copy must be contiguous")
            copies[by_id[id(p)]] = h
        return copies if any(h is not None for h in copies) else None

    @property
    def half_copies(self):
        """{parameter: fp16 working copy} the step writes, or {}"""
        if self._half is None:
            return {}
        return {p: h for p, h in zip(self._params, self._half) if h is not None}

    # ---- device scalars ------------------------------------------------------------------------------------------
    def _view(self, offset, dtype):
        return self._state_dev[offset:offset + torch.empty((), dtype=dtype).element_size()].view(dtype).reshape(())

    @property
    def step_tensor(self):
        """int64 device scalar: optimizer steps taken (skipped steps are not counted).  With neither clipping nor a loss
        scale the count is kept on the host (state_dict()['fused']['step'])."""
        return self._view(0, torch.int64)

    @property
    def skipped_steps(self):
        """int64 device scalar: steps skipped because the gradient norm was inf or NaN."""
        return self._view(8, torch.int64)

    @property
    def loss_scale_tensor(self):
        """fp32 device scalar: the loss scale the NEXT scale_loss() multiplies by."""
        return self._view(24, torch.float32)

    @property
    def last_grad_norm(self):
        """fp32 device scalar: the unscaled global gradient norm of the last step, before clipping (what
        clip_grad_norm_ returns).  Not computed with neither clipping nor a loss scale."""
        return self._view(28, torch.float32)

    @property
    def last_clip_coef(self):
        """fp32 device scalar: the clip coefficient of the last step, exactly 1 when nothing was clipped."""
        return self._view(56, torch.float32)

    def _init_device_state(self, step, scale, clean_steps, skipped):
        with torch.cuda.device(self._device):
            _lib.check(self._lib.proqa_adamw_state_init(self._state_dev.data_ptr(), int(step), float(scale), int(clean_steps),
                                                        int(skipped), _lib.current_stream_ptr()))

    def _refresh_static_pointers(self):
        self._table["p"] = [p.data_ptr() for p in self._params]
        self._table["m"] = [self.state[p]["exp_avg"].data_ptr() for p in self._params]
        self._table["v"] = [self.state[p]["exp_avg_sq"].data_ptr() for p in self._params]

    # ---- the loop's three calls ----------------------------------------------------------------------------------
    def scale_loss(self, loss):
        """loss * loss_scale as a device-side multiply (no synchronisation); the identity without a loss scale."""
        if self._scale_mode == _lib.ADAMW_SCALE_NONE:
            return loss
        return loss * self.loss_scale_tensor

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        table = self._table
        grads, lrs, wds = [], [], []
        for group in self.param_groups:
            lr, wd = float(group["lr"]), float(group["weight_decay"])
            for p in group["params"]:
                g = p.grad
                if g is None:
                    grads.append(0)
                else:
                    if g.dtype != torch.float32 or g.is_sparse or g.device != self._device or not g.is_contiguous() \
                            or g.numel() != p.numel():
                        raise RuntimeError("FusedAdamW takes dense contiguous fp32 gradients on the parameters' device")
                    grads.append(g.data_ptr())
                lrs.append(lr)
                wds.append(wd)
        if len(grads) != len(table):
            raise RuntimeError("FusedAdamW: parameters cannot be added after construction")
        table["g"], table["lr"], table["weight_decay"] = grads, lrs, wds
        hyper = _lib.AdamwHyper(beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                                max_grad_norm=self.max_grad_norm or 0.0, torch_semantics=int(self.torch_semantics),
                                scale_mode=self._scale_mode, backoff_factor=self.backoff_factor,
                                growth_factor=self.growth_factor, growth_interval=self.growth_interval,
                                host_step=self._plain_step + 1)
        with torch.cuda.device(self._device):
            # the table travels through pinned memory of torch's caching host allocator, which hands a block out again only
            # after the copy that read it has run: the host never waits for the stream, and never overwrites a table in use
            staged = torch.empty(table.nbytes, dtype=torch.uint8, pin_memory=True)
            staged.numpy()[:] = table.view(np.uint8)
            self._table_dev.copy_(staged, non_blocking=True)
            if self._half_dev is None:
                _lib.check(self._lib.proqa_adamw_step(self._table_dev.data_ptr(), len(table), self._chunks_dev.data_ptr(),
                                                      self._n_chunks, ctypes.byref(hyper), self._state_dev.data_ptr(),
                                                      self._ws.data_ptr(), self._ws.numel(), _lib.current_stream_ptr()))
            else:
                _lib.check(self._lib.proqa_adamw_step_half(self._table_dev.data_ptr(), self._half_dev.data_ptr(), len(table),
                                                           self._chunks_dev.data_ptr(), self._n_chunks, ctypes.byref(hyper),
                                                           self._state_dev.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                                           _lib.current_stream_ptr()))
        if self._plain:
            self._plain_step += 1
        return loss

    # ---- checkpoints (the only places that synchronise) ------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        if self._plain:
            fused = {"step": self._plain_step, "loss_scale": 1.0, "clean_steps": 0, "skipped_steps": 0}
        else:
            raw = self._state_dev.cpu().numpy()
            counters = raw[:24].view(np.int64)
            fused = {"step": int(counters[0]), "skipped_steps": int(counters[1]), "clean_steps": int(counters[2]),
                     "loss_scale": float(raw[24:28].view(np.float32)[0])}
        sd["fused"] = fused
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        fused = state_dict.pop("fused", None)
        if fused is None:
            raise ValueError("not a FusedAdamW state_dict: no 'fused' entry (step count and loss scale)")
        super().load_state_dict(state_dict)
        for p in self._params:       # torch re-creates the state tensors: back to contiguous fp32 on the device
            st = self.state[p]
            for k in ("exp_avg", "exp_avg_sq"):
                st[k] = st[k].to(device=self._device, dtype=torch.float32).contiguous()
        self._refresh_static_pointers()
        if self._plain:
            self._plain_step = int(fused["step"])
        else:
            scale = fused["loss_scale"] if self._scale_mode != _lib.ADAMW_SCALE_NONE else 1.0
            self._init_device_state(fused["step"], scale, fused["clean_steps"], fused["skipped_steps"])
