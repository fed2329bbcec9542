"""proqa_adamw_step_half and proqa_cast_half_tensors (csrc/optim_kernels.hip) through the C ABI.

The step with fp16 working copies must give p, m, v and the state the bits of proqa_adamw_step, and every copy the bits of
p.to(float16).  One table of 1, 3, 4, C-1, C, C+1 and 2C+5 elements (C = 16384, the chunk of one workgroup): chunk edges and
16-byte tails.  The tensor of C-1 elements has its fp32 storage offset by one element (the scalar path of p, g, m, v), the
one of C+1 has its COPY offset by one element (2-byte aligned: scalar 2-byte stores behind the 16-byte loop of p, g, m, v,
which keeps the bits the ordinary step gives that tensor), the one of 3 has
no gradient and the one of 4 has a NULL copy pointer.  There is no tolerance: every comparison is bitwise.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 16384
SIZES = [1, 3, 4, C - 1, C, C + 1, 2 * C + 5]
P_OFFSET, H_OFFSET, NO_GRAD, NO_COPY = 3, 5, 1, 2      # rows of the table
SCALE = 65536.0
GUARD = 0x7A5A      # the bit pattern planted around and behind the copies


def _hyper(_lib, max_grad_norm, scale_mode, torch_semantics, host_step=1):
    return _lib.AdamwHyper(beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=max_grad_norm, torch_semantics=int(torch_semantics),
                           scale_mode=scale_mode, backoff_factor=0.5, growth_factor=2.0, growth_interval=2000,
                           host_step=host_step)


class Table:
    """p, g, m, v, copies and the device tables of one optimizer over SIZES"""

    def __init__(self, dev, scale, bad=False):
        from proqa_amd import _lib
        from proqa_amd.optim import _TENSOR_DTYPE, _chunk_map
        self._lib, self.lib, self.dev = _lib, _lib.load(), dev
        gen = torch.Generator().manual_seed(11)
        self.p, self.g, self.m, self.v, self.h, self.h_store = [], [], [], [], [], []
        for i, n in enumerate(SIZES):
            off = 1 if i == P_OFFSET else 0

            def f32(values):
                buf = torch.zeros(n + off, device=dev)
                buf[off:] = values.to(dev)
                return buf[off:]
            self.p.append(f32(0.02 * torch.randn(n, generator=gen)))
            g = 0.01 * scale * torch.randn(n, generator=gen)
            if bad and i == 4:
                g[n // 2] = float("inf")
            self.g.append(None if i == NO_GRAD else f32(g))
            self.m.append(f32(0.001 * torch.randn(n, generator=gen)))
            self.v.append(f32(1e-4 * torch.rand(n, generator=gen)))
            # a copy with guard elements on both sides; the NULL row keeps its buffer to show that nothing writes it
            hoff = 9 if i == H_OFFSET else 8
            store = torch.full((n + 16,), GUARD, dtype=torch.int16, device=dev)
            self.h_store.append(store)
            self.h.append(store[hoff:hoff + n].view(torch.float16))
        assert self.p[P_OFFSET].data_ptr() % 16 == 4 and self.h[H_OFFSET].data_ptr() % 8 == 2 and self.h[0].data_ptr() % 8 == 0
        table = np.zeros(len(SIZES), dtype=_TENSOR_DTYPE)
        table["p"] = [t.data_ptr() for t in self.p]
        table["g"] = [0 if t is None else t.data_ptr() for t in self.g]
        table["m"] = [t.data_ptr() for t in self.m]
        table["v"] = [t.data_ptr() for t in self.v]
        table["n"] = SIZES
        table["lr"] = 1e-3
        table["weight_decay"] = [0.01 if i % 2 else 0.0 for i in range(len(SIZES))]
        self.table_dev = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
        chunks, self.n_chunks = _chunk_map(self.lib, np.array(SIZES, dtype=np.int64))
        assert self.n_chunks == 1 + 1 + 1 + 1 + 1 + 2 + 3
        self.chunks_dev = torch.from_numpy(chunks).to(dev)
        ptrs = np.array([0 if i == NO_COPY else h.data_ptr() for i, h in enumerate(self.h)], dtype=np.uint64)
        self.half_dev = torch.from_numpy(ptrs.view(np.int64)).to(dev)
        self.state = torch.zeros(_lib.ADAMW_STATE_BYTES, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(int(self.lib.proqa_adamw_workspace_bytes(self.n_chunks)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self.lib.proqa_adamw_state_init(self.state.data_ptr(), 0, float(scale), 0, 0, _lib.current_stream_ptr()))

    def step(self, hyper, half):
        _lib = self._lib
        with torch.cuda.device(self.dev):
            tail = (len(SIZES), self.chunks_dev.data_ptr(), self.n_chunks, ctypes.byref(hyper), self.state.data_ptr(),
                    self.ws.data_ptr(), self.ws.numel(), _lib.current_stream_ptr())
            if half:
                _lib.check(self.lib.proqa_adamw_step_half(self.table_dev.data_ptr(), self.half_dev.data_ptr(), *tail))
            else:
                _lib.check(self.lib.proqa_adamw_step(self.table_dev.data_ptr(), *tail))

    def cast(self):
        _lib = self._lib
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.proqa_cast_half_tensors(self.table_dev.data_ptr(), self.half_dev.data_ptr(), len(SIZES),
                                                        self.chunks_dev.data_ptr(), self.n_chunks, _lib.current_stream_ptr()))

    def bits(self):
        return ([t.cpu().view(torch.int32) for t in self.p], [t.cpu().view(torch.int32) for t in self.m],
                [t.cpu().view(torch.int32) for t in self.v], self.state.cpu())

    def stores(self):
        return [s.cpu() for s in self.h_store]


def _equal(a, b):
    """bitwise; prints which tensor of p, m, v (or the state) differs"""
    bad = [(name, i) for name, ta, tb in zip("pmv", a[:3], b[:3]) for i, (x, y) in enumerate(zip(ta, tb)) if not torch.equal(x, y)]
    if not torch.equal(a[3], b[3]):
        bad.append(("state", 0))
    if bad:
        print("different bits in (tensor, row of SIZES):", bad)
    return not bad


def _check_copies(t, before):
    """every copy is p.to(float16) bit for bit, except the row without a gradient (unchanged) and the NULL row (its buffer
    unchanged); the guard elements around every copy are untouched"""
    after = t.stores()
    for i, n in enumerate(SIZES):
        hoff = 9 if i == H_OFFSET else 8
        got = after[i][hoff:hoff + n]
        if i in (NO_GRAD, NO_COPY):
            assert torch.equal(after[i], before[i]), i
            continue
        want = t.p[i].cpu().to(torch.float16).view(torch.int16)
        assert torch.equal(got, want), (i, n)
        assert (after[i][:hoff] == GUARD).all() and (after[i][hoff + n:] == GUARD).all(), i


@pytest.mark.parametrize("mode", ["clip", "clip-torch", "plain", "plain-torch"])
def test_the_step_with_copies_changes_no_bit_of_the_step(gpu_device, mode):
    from proqa_amd import _lib
    plain, torch_semantics = mode.startswith("plain"), mode.endswith("torch")
    scale = 1.0 if plain else SCALE
    hyper = _hyper(_lib, 0.0 if plain else 1.0, _lib.ADAMW_SCALE_NONE if plain else _lib.ADAMW_SCALE_FIXED, torch_semantics)
    ref, got = Table(gpu_device, scale), Table(gpu_device, scale)
    assert _equal(ref.bits(), got.bits())
    before = got.stores()
    for k in range(2):
        hyper.host_step = k + 1
        ref.step(hyper, half=False)
        got.step(hyper, half=True)
    assert _equal(ref.bits(), got.bits())
    assert not torch.equal(got.p[4].cpu().view(torch.int32), Table(gpu_device, scale).p[4].cpu().view(torch.int32))
    if not plain:
        assert got.state.cpu()[:8].view(torch.int64).item() == 2
        assert got.state.cpu()[56:60].view(torch.float32).item() < 1.0       # the clip bites
    _check_copies(got, before)
    assert torch.equal(ref.stores()[0], before[0])       # proqa_adamw_step itself writes no copy


def test_half_dev_null_is_the_ordinary_step(gpu_device):
    from proqa_amd import _lib
    hyper = _hyper(_lib, 1.0, _lib.ADAMW_SCALE_FIXED, False)
    ref, got = Table(gpu_device, SCALE), Table(gpu_device, SCALE)
    before = got.stores()
    ref.step(hyper, half=False)
    got.half_dev = torch.zeros(0, dtype=torch.int64, device=gpu_device)     # data_ptr() == 0: NULL
    assert got.half_dev.data_ptr() == 0
    got.step(hyper, half=True)
    assert _equal(ref.bits(), got.bits())
    assert all(torch.equal(a, b) for a, b in zip(got.stores(), before))


def test_an_overflowing_step_writes_no_copy(gpu_device):
    from proqa_amd import _lib
    hyper = _hyper(_lib, 1.0, _lib.ADAMW_SCALE_DYNAMIC, False)
    t = Table(gpu_device, SCALE, bad=True)
    p0, stores0 = t.bits(), t.stores()
    t.step(hyper, half=True)
    after = t.bits()
    assert all(torch.equal(x, y) for a, b in zip(after[:3], p0[:3]) for x, y in zip(a, b))
    assert after[3][8:16].view(torch.int64).item() == 1 and after[3][24:28].view(torch.float32).item() == 32768.0
    assert all(torch.equal(a, b) for a, b in zip(t.stores(), stores0))


def test_cast_half_tensors_rounds_as_torch_does(gpu_device):
    t = Table(gpu_device, 1.0)
    planted = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,       # the two ties of round-to-nearest-even
                            65504.0, 65519.99, 65520.0,               # the largest, just below the tie to inf, the tie
                            6e-8, 2.98e-8,                            # a subnormal, the tie below the smallest one
                            -0.0, float("inf"), float("-inf"), float("nan"),
                            -(1 + 2.0 ** -11), -65520.0, 2.0 ** -25 * (1 + 2.0 ** -20), 1e-30, 3.0e38], dtype=torch.float32)
    assert planted[1].item() == 1 + 3 * 2.0 ** -11 and planted.numel() == 16
    with torch.no_grad():
        for i in (4, 5, 6):       # 16-byte path, 2-byte aligned copy, and a tail after two full chunks
            t.p[i][:16] = planted.to(gpu_device)
            t.p[i][-5:] = planted[:5].to(gpu_device)
        t.p[P_OFFSET][:16] = planted.to(gpu_device)
    before = t.stores()
    masters = [p.clone() for p in t.p]
    t.cast()
    after = t.stores()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(t.p, masters))     # the masters are only read
    for i, n in enumerate(SIZES):
        hoff = 9 if i == H_OFFSET else 8
        if i == NO_COPY:
            assert torch.equal(after[i], before[i])
            continue
        got = after[i][hoff:hoff + n]
        want = t.p[i].cpu().to(torch.float16)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got.view(torch.float16)), nan), i          # NaN out, any payload
        assert torch.equal(got[~nan], want.view(torch.int16)[~nan]), i
        assert (after[i][:hoff] == GUARD).all() and (after[i][hoff + n:] == GUARD).all(), i
    got = after[4][8:8 + 16].view(torch.float16)
    assert got[0].item() == 1.0 and got[1].item() == 1 + 2.0 ** -9 and got[3].item() == 65504.0 and got[4].item() == float("inf")
    assert got[5].view(torch.int16).item() == 1 and got[6].view(torch.int16).item() == 0
    assert got[7].view(torch.int16).item() == -32768 and torch.isnan(got[10]).item()


def test_arguments_are_checked(gpu_device):
    from proqa_amd import _lib
    t = Table(gpu_device, 1.0)
    rc = t.lib.proqa_cast_half_tensors(t.table_dev.data_ptr(), None, len(SIZES), t.chunks_dev.data_ptr(), t.n_chunks, None)
    assert rc != 0
    with pytest.raises(Exception, match="cast_half_tensors"):
        _lib.check(rc)
