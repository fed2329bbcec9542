"""proqa_reader_loss_f16 / proqa_reader_loss_backward_f16 and proqa_amd.reader_loss against the float64 restatement
(tests/reader_loss_oracle.py, itself held to the reference's BertRetrieveQA.forward by tests/test_reader_loss_host.py).

Error measure: max|gpu - ref| / max|ref| per output against float64.  Bound: four times the same measure of the oracle's
storage="fp16" mode (fp16 logits, fp16 d_hidden and d_q, float32 elsewhere: the reference's arithmetic under apex O1),
the maximum over the four (norm, early) variants of a case.  Measured on the CPU by measure_reference_error() (the host
test reproduces the table):

    case                 loss     logits   d_hidden     d_qa_w     d_qa_b        d_q
    ragged128       1.607e-04  3.296e-04  4.069e-04  5.326e-04  5.364e-07  4.748e-04
    ragged768       1.614e-05  3.204e-04  4.084e-04  2.841e-04  3.129e-07  3.972e-04
    p_equals_b      8.124e-05  2.925e-04  5.938e-04  6.448e-04  4.619e-07  4.479e-04
    long768         4.802e-05  2.749e-04  5.071e-04  5.545e-04  4.470e-07  3.547e-04
    onerow          1.377e-07  4.402e-04  0.000e+00  0.000e+00  0.000e+00  2.514e-04
    logits40        7.438e-05  2.955e-04  6.409e-04  3.303e-04  3.997e-06  2.976e-04
    dropout         1.996e-04  3.352e-04  7.264e-04  7.601e-04  3.204e-07  3.627e-04

Where a float64 gradient vanishes by cancellation (below 1e-6 of its operands: the one-row paragraph, whose softmax is 1
and whose pair weight is 1) the error is taken relative to the operands instead: max|qa_w| for d_hidden, max|hidden| for
d_qa_w, 1 for d_qa_b.  Outputs that are exactly zero in float64 (nothing valid: no term of the loss is live) must be
exactly zero on the GPU.

Twenty FusedAdamW steps (lr 5e-2, dynamic loss scale) on qa_weight, qa_bias and a free hidden tensor of the "ragged128"
case: initial loss 14.679, float64 restatement after 20 steps 4.772 (train_trajectory(), CPU); the GPU has to get
below their geometric mean.
"""
import ctypes
import functools
import math

import pytest
import torch

import adamw_oracle
import reader_loss_oracle as oracle

pytestmark = pytest.mark.gpu

OUTPUTS = oracle.OUTPUTS
REFERENCE_ERROR = {
    "ragged128": dict(zip(OUTPUTS, [0.0001607, 0.0003296, 0.0004069, 0.0005326, 5.364e-07, 0.0004748])),
    "ragged768": dict(zip(OUTPUTS, [1.614e-05, 0.0003204, 0.0004084, 0.0002841, 3.129e-07, 0.0003972])),
    "p_equals_b": dict(zip(OUTPUTS, [8.124e-05, 0.0002925, 0.0005938, 0.0006448, 4.619e-07, 0.0004479])),
    "long768": dict(zip(OUTPUTS, [4.802e-05, 0.0002749, 0.0005071, 0.0005545, 4.47e-07, 0.0003547])),
    "onerow": dict(zip(OUTPUTS, [1.377e-07, 0.0004402, 0.0, 0.0, 0.0, 0.0002514])),
    "logits40": dict(zip(OUTPUTS, [7.438e-05, 0.0002955, 0.0006409, 0.0003303, 3.997e-06, 0.0002976])),
    "dropout": dict(zip(OUTPUTS, [0.0001996, 0.0003352, 0.0007264, 0.0007601, 3.204e-07, 0.0003627])),
}
TRAIN_LR = 5e-2
TRAIN_L0, TRAIN_L20 = 14.679292913053835, 4.771903536339161

VARIANTS = [(True, True), (True, False), (False, True), (False, False)]       # (shared_norm, early)
SEED, CALL, SITE = 0x1234_5678_9ABC_DEF0, 7, 255
RAGGED = dict(lens=[40, 33, 25, 40, 12, 9], para_offset=[6, 9, 5, 12, 7, 8],            # the last paragraph is empty
              start=[[10, 10, 20], [9, 3, -1], [23, -1, -1], [-1, -1, -1], [8, 10, -1], [8, -1, -1]],
              end=[[12, 12, 25], [31, 10, -1], [23, -1, -1], [-1, -1, -1], [10, 11, -1], [8, -1, -1]])
LONG = dict(lens=[512, 512, 500, 512, 301, 512], para_offset=[10, 14, 9, 20, 12, 11],
            start=[[400, 400, 33], [14, 5, -1], [498, -1, -1], [-1, -1, -1], [299, 100, -1], [64, 511, -1]],
            end=[[410, 410, 40], [510, 20, -1], [498, -1, -1], [-1, -1, -1], [299, 300, -1], [96, 511, -1]])
ONEROW = dict(lens=[8], para_offset=[6], start=[[6, -1, -1]], end=[[6, -1, -1]])
CASES = {
    # name: geometry, H, P, para dtype, scale of the hidden states, dropout rate
    "ragged128": (RAGGED, 128, 300, torch.float16, 1.0, 0.0),
    "ragged768": (RAGGED, 768, 5000, torch.float32, 1.0, 0.0),
    "p_equals_b": (RAGGED, 128, 6, torch.float16, 1.0, 0.0),
    "long768": (LONG, 768, 300, torch.float16, 1.0, 0.0),
    "onerow": (ONEROW, 128, 3, torch.float16, 1.0, 0.0),
    "logits40": (RAGGED, 128, 300, torch.float16, 4.0, 0.0),
    "dropout": (RAGGED, 128, 300, torch.float16, 1.0, 0.1),
}
CANCEL = 1e-6


def host_keep(p, lens, L, H):
    """[B, L, H] bool: proqa_dropout_keep_host at (packed row, column), site 255"""
    from proqa_amd import _lib
    lib = _lib.load()
    keep = torch.zeros((len(lens), L, H), dtype=torch.bool)
    buf = (ctypes.c_uint8 * H)()
    row = 0
    for b, n in enumerate(lens):
        for t in range(n):
            _lib.check(lib.proqa_dropout_keep_host(0, p, SEED, SITE, CALL, row, 0, 0, H, buf))
            keep[b, t] = torch.tensor(list(buf), dtype=torch.bool)
            row += 1
    return keep


@functools.lru_cache(maxsize=None)
def make_case(name):
    geo, H, P, para_dtype, scale, p = CASES[name]
    lens = geo["lens"]
    B, L = len(lens), max(lens)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    hidden = (scale * torch.randn(B, L, H, generator=g)).half()
    for b, n in enumerate(lens):
        hidden[b, n:] = 0
    para = 0.4 * torch.randn(P, 128, generator=g)
    para = para.half() if para_dtype == torch.float16 else para
    labels = torch.zeros(P, dtype=torch.int64)
    labels[[0, P // 2, P - 1]] = 1                    # an index below B, and the last one
    c = dict(hidden=hidden, qa_w=(0.3 * torch.randn(2, H, generator=g) / math.sqrt(H / 128)).half(),
             qa_b=(0.1 * torch.randn(2, generator=g)).half(), q=(0.4 * torch.randn(128, generator=g)).half(), para=para,
             labels=labels, start=torch.tensor(geo["start"]), end=torch.tensor(geo["end"]), lens=lens,
             para_offset=geo["para_offset"], keep=None, factor=1.0)
    if p > 0:
        thr = min(65535, math.floor(p * 65536 + 0.5))
        c["keep"] = host_keep(p, lens, L, H)
        c["factor"] = float(torch.tensor(1.0, dtype=torch.float32) / (1.0 - torch.tensor(thr / 65536.0, dtype=torch.float32)))
    return c


@functools.lru_cache(maxsize=None)
def reference(name, shared_norm, early, grad=1.0):
    return oracle.evaluate(**make_case(name), shared_norm=shared_norm, early=early, grad=grad)


def valid_rows(c):
    m = torch.zeros(c["hidden"].shape[:2], dtype=torch.bool)
    for b, n in enumerate(c["lens"]):
        m[b, :n] = True
    return m


def errors(c, got, ref):
    """{output: error}; the rule of the header for gradients that vanish by cancellation"""
    rows = valid_rows(c)
    operand = {"d_hidden": float(c["qa_w"].abs().max()), "d_qa_w": float(c["hidden"].abs().max()), "d_qa_b": 1.0}
    out = {}
    for k in oracle.OUTPUTS:
        g, r = (got[k][rows], ref[k][rows]) if k in ("logits", "d_hidden") else (got[k], ref[k])
        top = float(r.abs().max()) if r.numel() else 0.0
        floor = operand[k] if k in operand and top < CANCEL * operand[k] else 0.0
        out[k] = oracle.error(g, r, floor)
    return out


def measure_reference_error():
    """{case: {output: error of the storage="fp16" mode against float64, the maximum over VARIANTS}}"""
    table = {}
    for name in CASES:
        c = make_case(name)
        worst = {k: 0.0 for k in oracle.OUTPUTS}
        for shared_norm, early in VARIANTS:
            half = oracle.evaluate(**c, shared_norm=shared_norm, early=early, storage="fp16")
            for k, v in errors(c, half, reference(name, shared_norm, early)).items():
                worst[k] = max(worst[k], v)
        table[name] = worst
    return table


def train_trajectory(steps=20):
    """(initial loss, loss after `steps` float64 AdamW steps) on qa_w, qa_b and the hidden states of "ragged128" """
    c = dict(make_case("ragged128"))
    params = [c["hidden"].double(), c["qa_w"].double(), c["qa_b"].double()]
    ms, vs = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    state, hp = adamw_oracle.new_state(), adamw_oracle.hyper()
    losses = []
    for _ in range(steps + 1):
        c.update(hidden=params[0], qa_w=params[1], qa_b=params[2])
        out = oracle.evaluate(**c)
        losses.append(float(out["loss"]))
        grads = [out["d_hidden"], out["d_qa_w"], out["d_qa_b"]]
        state, params, ms, vs, _ = adamw_oracle.oracle_step(state, hp, params, grads, ms, vs, [TRAIN_LR] * 3, [0.0] * 3)
    return losses[0], losses[steps]


# ---- running the library ---------------------------------------------------------------------------------------------------

def device_case(c, dev, packed):
    from proqa_amd import reader_loss as RL
    lens = c["lens"]
    B, L, H = c["hidden"].shape
    if packed:
        hidden = torch.cat([c["hidden"][b, :n] for b, n in enumerate(lens)]).to(dev)
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)
        layout = dict(cu_seqlens=cu, seq_lens=None, max_seq_len=L)
    else:
        hidden = c["hidden"].to(dev)
        layout = dict(cu_seqlens=None, seq_lens=torch.tensor(lens, dtype=torch.int32, device=dev), max_seq_len=None)
    return RL, hidden, layout


def run(c, dev, shared_norm=True, early=True, grad=1.0, packed=True, p=None):
    """forward + backward through the tensor-in / tensor-out layer -> outputs on the CPU, hidden-shaped ones padded
    [B, L, .] (rows the library does not own are NaN in the packed run)"""
    RL, hidden, layout = device_case(c, dev, packed)
    B, L, H = c["hidden"].shape
    p = rate_of(c) if p is None else p
    geo = RL._Geometry(hidden, layout["cu_seqlens"], layout["seq_lens"], torch.tensor(c["para_offset"], device=dev),
                       c["start"].to(dev), c["end"].to(dev), c["para"].to(dev), c["labels"].to(dev), shared_norm, early, p,
                       (SEED, CALL), layout["max_seq_len"])
    w16, b16, q = c["qa_w"].to(dev), c["qa_b"].to(dev), c["q"].to(dev)
    loss_out, logits, stats = RL.reader_loss_forward(hidden, w16, b16, q, geo)
    g = torch.tensor([grad], dtype=torch.float32, device=dev)
    d_hidden, d_w, d_b, d_q = RL.reader_loss_backward(hidden, w16, q, geo, logits, stats, g)

    def padded(x, width):
        x = x.cpu()
        if not packed:
            return x.reshape(B, L, width)
        out = torch.full((B, L, width), float("nan"), dtype=x.dtype)
        row = 0
        for b, n in enumerate(c["lens"]):
            out[b, :n] = x[row:row + n]
            row += n
        return out
    lo = loss_out.cpu()
    return dict(loss=lo[0], joint=lo[1], early=lo[2], logits=padded(logits, 2), d_hidden=padded(d_hidden, H),
                d_qa_w=d_w.cpu(), d_qa_b=d_b.cpu(), d_q=d_q.cpu(), stats=stats.cpu())


def rate_of(c):
    return 0.1 if c["keep"] is not None else 0.0


def same_bits(a, b, keys=("loss", "logits", "d_hidden", "d_qa_w", "d_qa_b", "d_q")):
    def bits(x):
        return x.contiguous().view(torch.int16 if x.dtype == torch.float16 else torch.int32)
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in keys)


def check(name, c, got, ref, what=""):
    errs = errors(c, got, ref)
    for k, e in errs.items():
        bound = 4.0 * REFERENCE_ERROR[name][k]
        print(f"{name}{what} {k}: error {e:.3e} bound {bound:.3e}")
    for k, e in errs.items():
        if float(ref[k].abs().max()) == 0.0:
            assert float(got[k][torch.isfinite(got[k])].abs().max()) == 0.0, f"{name}{what} {k}: exactly zero in float64"
        else:
            assert e <= 4.0 * REFERENCE_ERROR[name][k], f"{name}{what} {k}: error {e:.3e} over 4 x {REFERENCE_ERROR[name][k]:.3e}"


# ---- the bounds, every case and variant -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shared_norm,early", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_against_float64(gpu_device, name, shared_norm, early):
    c, ref = make_case(name), reference(name, shared_norm, early)
    got = run(c, gpu_device, shared_norm, early)
    check(name, c, got, ref)
    assert abs(float(got["loss"]) - float(got["joint"]) - float(got["early"])) <= 1e-6 * max(1.0, abs(float(got["loss"])))
    if not early:
        assert float(got["early"]) == 0.0
    # rows outside the paragraph mask carry no gradient: exactly zero
    outside = valid_rows(c) & ~oracle._mask(c["hidden"].shape[1], c["lens"], c["para_offset"])
    assert (got["d_hidden"][outside] == 0).all()


def test_degenerate_batches(gpu_device):
    base = make_case("ragged128")
    none = torch.full_like(base["start"], -1)
    no_pair = dict(base, start=none, end=none)
    no_gold = dict(base, labels=torch.zeros_like(base["labels"]))
    neither = dict(no_pair, labels=torch.zeros_like(base["labels"]))
    for shared_norm in (True, False):
        for what, c in (("no pair", no_pair), ("no gold", no_gold)):
            got, ref = run(c, gpu_device, shared_norm), oracle.evaluate(**c, shared_norm=shared_norm)
            check("ragged128", c, got, ref, f" ({what})")
            assert float(got["joint" if what == "no pair" else "early"]) == 0.0
        got = run(neither, gpu_device, shared_norm)
        assert float(got["loss"]) == 0.0
        for k in ("d_hidden", "d_qa_w", "d_qa_b", "d_q"):
            assert (got[k][torch.isfinite(got[k])] == 0).all() and torch.isfinite(got[k]).sum() > 0, k


def test_logits_are_reader_spans_bits(gpu_device):
    from proqa_amd import _lib
    lib = _lib.load()
    for name in ("ragged128", "ragged768", "logits40"):
        c = make_case(name)
        got = run(c, gpu_device)
        RL, hidden, layout = device_case(c, gpu_device, True)
        B = len(c["lens"])
        outs = [torch.empty(B, dtype=t, device=gpu_device) for t in (torch.int32, torch.int32, torch.float32)]
        logits = torch.zeros((hidden.shape[0], 2), dtype=torch.float16, device=gpu_device)
        w16, b16 = c["qa_w"].to(gpu_device), c["qa_b"].to(gpu_device)
        offs = torch.tensor(c["para_offset"], dtype=torch.int32, device=gpu_device)
        _lib.check(lib.proqa_reader_span_f16(hidden.data_ptr(), None, layout["cu_seqlens"].data_ptr(), B, max(c["lens"]),
                                             hidden.shape[1], offs.data_ptr(), w16.data_ptr(), b16.data_ptr(), 5,
                                             outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), logits.data_ptr(),
                                             _lib.current_stream_ptr()))
        torch.cuda.synchronize()
        mine = got["logits"][valid_rows(c)]
        assert torch.equal(mine.view(torch.int16), logits.cpu().view(torch.int16))


def test_dropout_mask_is_the_host_functions(gpu_device):
    c = make_case("dropout")
    # an incoming gradient of 2^12 (a loss scale) keeps the smallest probabilities' gradients above fp16's underflow
    got = run(c, gpu_device, grad=4096.0)
    mask = oracle._mask(c["hidden"].shape[1], c["lens"], c["para_offset"])
    # inside the paragraph mask d_hidden is zero exactly where the element was dropped
    assert torch.equal(got["d_hidden"][mask] != 0, c["keep"][mask])
    assert 0.05 < 1.0 - float(c["keep"][mask].float().mean()) < 0.15
    # and without dropout nothing is zero there
    assert (run(dict(c, keep=None, factor=1.0), gpu_device, grad=4096.0)["d_hidden"][mask] != 0).all()


def test_padded_and_packed_layouts_agree(gpu_device):
    for name in ("ragged128", "dropout"):
        c = make_case(name)
        a, b = run(c, gpu_device, packed=True), run(c, gpu_device, packed=False)
        rows = valid_rows(c)
        assert same_bits(a, b, keys=("loss", "d_qa_w", "d_qa_b", "d_q"))
        for k in ("logits", "d_hidden"):
            assert torch.equal(a[k][rows].view(torch.int16), b[k][rows].view(torch.int16))
        assert (b["d_hidden"][~rows] == 0).all() and (b["logits"][~rows] == 0).all()


def test_linear_in_the_incoming_gradient(gpu_device):
    """x 1024: exactly 1024 x the fp32 outputs, and the fp16 outputs wherever the value at 1 is a normal fp16 number (a
    subnormal holds fewer bits than its image); inf: non-finite outputs, and the call returns"""
    c = make_case("ragged128")
    one, big = run(c, gpu_device), run(c, gpu_device, grad=1024.0)
    for k in ("d_qa_w", "d_qa_b"):
        assert torch.equal(big[k], one[k] * 1024.0), k
    for k in ("d_hidden", "d_q"):
        a, b = one[k][torch.isfinite(one[k])].float(), big[k][torch.isfinite(big[k])].float()
        normal = a.abs() >= 2.0 ** -14
        assert normal.any() and torch.equal(b[normal], a[normal] * 1024.0), k
        assert ((b - a * 1024.0).abs() <= 1024.0 * 2.0 ** -25).all(), k          # (half a step of fp16's subnormals)
    outside = valid_rows(c) & ~oracle._mask(c["hidden"].shape[1], c["lens"], c["para_offset"])
    assert (big["d_hidden"][outside] == 0).all()
    bad = run(c, gpu_device, grad=float("inf"))
    torch.cuda.synchronize()
    for k in ("d_hidden", "d_qa_w", "d_qa_b", "d_q"):
        assert not torch.isfinite(bad[k][valid_rows(c)] if k == "d_hidden" else bad[k]).all(), k
    assert same_bits(one, run(c, gpu_device))


def test_two_runs_have_the_same_bits(gpu_device):
    for name in ("ragged768", "long768", "dropout"):
        c = make_case(name)
        assert same_bits(run(c, gpu_device), run(c, gpu_device))
        assert same_bits(run(c, gpu_device, False, True), run(c, gpu_device, False, True))


def api_inputs(c, dev):
    hidden = torch.cat([c["hidden"][b, :n] for b, n in enumerate(c["lens"])]).to(dev).requires_grad_(True)
    cu = torch.tensor([0] + list(torch.tensor(c["lens"]).cumsum(0)), dtype=torch.int32, device=dev)
    w = c["qa_w"].float().to(dev).requires_grad_(True)
    b = c["qa_b"].float().to(dev).requires_grad_(True)
    rest = dict(para_embed=c["para"].to(dev), top5000_labels=c["labels"].to(dev), start_positions=c["start"].to(dev),
                end_positions=c["end"].to(dev), para_offset=torch.tensor(c["para_offset"], device=dev), cu_seqlens=cu,
                max_seq_len=max(c["lens"]))
    return hidden, w, b, rest


def test_autograd_function_without_a_host_wait(gpu_device):
    from proqa_amd.reader_loss import reader_loss
    c, ref = make_case("ragged128"), reference("ragged128", True, True)
    hidden, w, b, rest = api_inputs(c, gpu_device)
    q = c["q"].to(gpu_device).requires_grad_(True)
    reader_loss(hidden, w, b, q, **rest)["loss"].backward()          # (the workspace is allocated here, not under the guard)
    for t in (hidden, w, b, q):
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = reader_loss(hidden, w, b, q, **rest)
        out["loss"].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert w.grad.dtype == torch.float32 and b.grad.dtype == torch.float32
    assert hidden.grad.dtype == torch.float16 and q.grad.dtype == torch.float16
    low = run(c, gpu_device)
    assert torch.equal(hidden.grad.cpu(), low["d_hidden"][valid_rows(c)]) and torch.equal(q.grad.cpu(), low["d_q"])
    assert torch.equal(w.grad.cpu(), low["d_qa_w"]) and torch.equal(b.grad.cpu(), low["d_qa_b"])
    assert float(out["loss"].detach()) == float(low["loss"]) and not out["joint"].requires_grad
    assert oracle.error(out["loss"].detach().cpu(), ref["loss"]) <= 4.0 * REFERENCE_ERROR["ragged128"]["loss"]


def test_question_tower_receives_the_gradient(gpu_device):
    import train_oracle
    from proqa_amd.reader_loss import reader_loss
    from proqa_amd.trainable import TrainableRetriever
    model = TrainableRetriever(train_oracle.SMALL_CONFIG, device=gpu_device).train()
    c = make_case("ragged128")
    hidden, w, b, rest = api_inputs(c, gpu_device)
    B = len(c["lens"])
    ids = torch.randint(1, 100, (B, 9), generator=torch.Generator().manual_seed(5)).to(gpu_device)      # B identical-length rows
    ids[1:] = ids[0]
    q = model.get_embed({"input_ids": ids, "input_mask": torch.ones_like(ids)}, True)["embed"]
    out = reader_loss(hidden, w, b, q, **rest)
    (out["loss"] * 256.0).backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    mine = [g for k, g in grads.items() if k.startswith(("bert_q.", "proj_q."))]
    assert all(g is not None and torch.isfinite(g).all() for g in mine) and any((g != 0).any() for g in mine)
    assert all(g is None for k, g in grads.items() if k.startswith(("bert_c.", "proj_c.")))


def test_twenty_fused_adamw_steps_reduce_the_loss(gpu_device):
    from proqa_amd.optim import FusedAdamW
    from proqa_amd.reader_loss import reader_loss
    c = make_case("ragged128")
    hidden16, w, b, rest = api_inputs(c, gpu_device)
    master = hidden16.detach().float().requires_grad_(True)
    q = c["q"].to(gpu_device)
    opt = FusedAdamW([master, w, b], lr=TRAIN_LR, loss_scale="dynamic")
    losses = []
    for _ in range(21):
        out = reader_loss(master.half(), w, b, q, **rest)
        losses.append(out["loss"].detach())
        opt.zero_grad()
        opt.scale_loss(out["loss"]).backward()
        opt.step()
    losses = [float(v) for v in losses]
    print("losses", losses[0], losses[20], "float64", TRAIN_L0, TRAIN_L20)
    assert abs(losses[0] - TRAIN_L0) <= 1e-2 * TRAIN_L0
    assert losses[20] < math.sqrt(TRAIN_L0 * TRAIN_L20)
