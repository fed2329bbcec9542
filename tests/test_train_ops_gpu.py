"""The backward operators of csrc/train_kernels.hip against tests/train_oracle.py (torch.autograd in float64 on the kernels'
own fp16 inputs).

Error measure, per output tensor: max|gpu - ref| / max|ref|.

Tolerance: four times the same measure of the oracle's storage="fp16" mode (fp32 arithmetic, fp16 wherever the module
stores fp16: the reference's own arithmetic under apex O1) against float64, the maximum over the cases of an operator --
measure_reference_error() below, run on the CPU.  The factor 4 is what this project gives device intrinsics and
re-associated sums over libm (tests/test_inbatch_gpu.py, K_INTRINSICS).  Measured (REFERENCE_ERROR) and allowed (BOUNDS):

    operator                      output     measured    bound
    attention backward            d_qkv      5.485e-04   2.194e-03
    bias+residual+LayerNorm bwd   dz         3.271e-04   1.308e-03
                                  dgamma     1.631e-07   6.524e-07
                                  dbeta      7.284e-08   2.914e-07
                                  dbias      1.638e-07   6.552e-07
    bias+GELU backward            dx         3.883e-04   1.553e-03
                                  dbias      1.832e-07   7.328e-07
    embedding+LayerNorm backward  dgamma     1.794e-07   7.176e-07
                                  dbeta      4.544e-08   1.818e-07
                                  d_word     1.449e-07   5.796e-07
                                  d_pos      1.273e-07   5.092e-07
                                  d_type0    1.526e-07   6.104e-07
    in-batch loss gradient        dq         4.162e-04   1.665e-03
                                  dc         2.402e-04   9.608e-04
    column sum                    out        6.849e-08   2.740e-07

The key third of the attention's bias gradient (exactly zero in the oracle) is held to the d_qkv bound relative to the
whole bias gradient.  The (1, 1) loss case has a zero gradient: there the error is taken relative to max|c| (dq) and
max|q| (dc), the size of the terms that cancel.
"""
import functools

import numpy as np
import pytest
import torch

import train_oracle as oracle
from test_inbatch_gpu import gaussian_case

pytestmark = pytest.mark.gpu

REFERENCE_ERROR = {
    "attention": {"d_qkv": 5.485e-04},
    "layernorm": {"dz": 3.271e-04, "dgamma": 1.631e-07, "dbeta": 7.284e-08, "dbias": 1.638e-07},
    "gelu": {"dx": 3.883e-04, "dbias": 1.832e-07},
    "embed": {"dgamma": 1.794e-07, "dbeta": 4.544e-08, "d_word": 1.449e-07, "d_pos": 1.273e-07, "d_type0": 1.526e-07},
    "loss": {"dq": 4.162e-04, "dc": 2.402e-04},
    "colsum": {"out": 6.849e-08},
}
BOUNDS = {op: {k: 4.0 * v for k, v in d.items()} for op, d in REFERENCE_ERROR.items()}


def rng_f16(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).half()


# ---- cases (CPU tensors; the float64 reference of each is computed once) ----------------------------------------------------

ATTENTION_BATCHES = {"one": [1], "ragged": [17, 64, 65, 128, 129, 3], "long": [200, 512, 1]}
ATTENTION_CASES = [(2, "one"), (2, "ragged"), (2, "long"), (12, "ragged")]


@functools.lru_cache(maxsize=None)
def attention_case(n_heads, batch, with_bias, q_scale=1.0):
    lens = ATTENTION_BATCHES[batch]
    T, H = sum(lens), 64 * n_heads
    seed = 1000 * n_heads + T
    qkv = rng_f16(seed, T, 3 * H)
    if q_scale != 1.0:
        qkv[:, :H] = (qkv[:, :H].float() * q_scale).half()
    bias = rng_f16(seed + 1, 3 * H, scale=0.5) if with_bias else None
    d_ctx = rng_f16(seed + 2, T, H)
    ref = oracle.attention_backward(qkv, bias, d_ctx, lens, n_heads)
    return dict(qkv=qkv, bias=bias, d_ctx=d_ctx, lens=lens, n_heads=n_heads), ref


LAYERNORM_CASES = [(1, 128, 1.0), (37, 128, 1.0), (300, 768, 1.0), (513, 768, 1.0), (300, 768, 1e3)]


@functools.lru_cache(maxsize=None)
def layernorm_case(rows, cols, magnitude):
    seed = rows * 7 + cols + int(magnitude)
    c = dict(dy=rng_f16(seed, rows, cols), x=rng_f16(seed + 1, rows, cols, scale=magnitude),
             bias=rng_f16(seed + 2, cols, scale=0.1), residual=rng_f16(seed + 3, rows, cols, scale=magnitude),
             gamma=(1.0 + 0.1 * torch.randn(cols, generator=torch.Generator().manual_seed(seed + 4))).half(), eps=1e-12)
    return c, oracle.bias_residual_layernorm_backward(**c)


GELU_CASES = [(37, 512), (300, 3072)]
GELU_SPECIALS = (0.0, 8.0, -8.0, 6e4, -6e4)


@functools.lru_cache(maxsize=None)
def gelu_case(rows, cols):
    seed = rows + cols
    x = rng_f16(seed, rows, cols, scale=1.5)
    bias = rng_f16(seed + 1, cols, scale=0.1)
    bias[:8] = 0
    for i, v in enumerate(GELU_SPECIALS):       # x_pre + bias is exactly the special value
        x[i % rows, i] = v
        x[rows - 1, i] = v
    c = dict(dy=rng_f16(seed + 2, rows, cols), x_pre=x, bias=bias)
    return c, oracle.bias_gelu_backward(**c)


EMBED_CASES = [(128, (64, 37, 80, 1, 55, 63)), (768, (64, 37, 80, 1, 55, 63))]
EMBED_VOCAB, EMBED_USED, EMBED_POSITIONS = 50, 45, 96


@functools.lru_cache(maxsize=None)
def embed_case(hidden, lens):
    """vocabulary 50, T = 300 in six sequences: ids repeat heavily.  Ids 45 .. 49 appear only PAST the lengths."""
    g = torch.Generator().manual_seed(hidden)
    S = max(lens)
    ids = torch.randint(0, EMBED_USED, (len(lens), S), generator=g)
    pad = torch.arange(S)[None] >= torch.tensor(lens)[:, None]
    ids[pad] = torch.randint(EMBED_USED, EMBED_VOCAB, (int(pad.sum()),), generator=g)
    c = dict(dy=rng_f16(hidden + 1, sum(lens), hidden), ids=ids, lens=lens, word=rng_f16(hidden + 2, EMBED_VOCAB, hidden),
             pos=rng_f16(hidden + 3, EMBED_POSITIONS, hidden), type0=rng_f16(hidden + 4, hidden),
             gamma=(1.0 + 0.1 * torch.randn(hidden, generator=g)).half(), eps=1e-12)
    return c, oracle.embed_layernorm_backward(**c)


LOSS_CASES = ["one", "duplicates", "gaussian100", "gaussian300"]


@functools.lru_cache(maxsize=None)
def loss_case(name):
    if name == "one":
        q, c, target = rng_f16(1, 1, 128), rng_f16(2, 1, 128), None
    elif name == "duplicates":
        q, c = rng_f16(3, 33, 128, scale=0.3), rng_f16(4, 65, 128, scale=0.3)
        target = torch.randint(0, 65, (33,), generator=torch.Generator().manual_seed(5)).int()
        target[:6] = torch.tensor([7, 7, 7, 0, 64, 64]).int()            # several questions share a target
    else:
        q, c, target = gaussian_case(*{"gaussian100": (100, 100), "gaussian300": (300, 777)}[name])
        q, c = torch.from_numpy(q), torch.from_numpy(c)
        target = None if target is None else torch.from_numpy(target)
    return dict(q=q, c=c, target=target), oracle.inbatch_loss_grad(q, c, target)


COLSUM_CASES = [(1, 128), (513, 2304)]


def measure_reference_error():
    """{operator: {output: max over the cases of rel_err(storage='fp16' oracle, float64 oracle)}} -- CPU only; the table
    in the header and REFERENCE_ERROR are its output."""
    worst = {}

    def note(op, got, ref):
        for k in ref:
            worst.setdefault(op, {})[k] = max(worst.get(op, {}).get(k, 0.0), oracle.rel_err(got[k], ref[k]))

    kw = dict(dtype=torch.float32, storage="fp16")
    for n_heads, batch in ATTENTION_CASES:
        for with_bias in (True, False):
            c, ref = attention_case(n_heads, batch, with_bias)
            note("attention", oracle.attention_backward(c["qkv"], c["bias"], c["d_ctx"], c["lens"], c["n_heads"], **kw), ref)
    for case in LAYERNORM_CASES:
        c, ref = layernorm_case(*case)
        note("layernorm", oracle.bias_residual_layernorm_backward(**c, **kw), ref)
    for case in GELU_CASES:
        c, ref = gelu_case(*case)
        note("gelu", oracle.bias_gelu_backward(**c, **kw), ref)
    for case in EMBED_CASES:
        c, ref = embed_case(*case)
        note("embed", oracle.embed_layernorm_backward(**c, **kw), ref)
    for name in LOSS_CASES[1:]:                 # (the (1, 1) gradient is zero)
        c, ref = loss_case(name)
        note("loss", oracle.inbatch_loss_grad(**c, **kw), ref)
    for rows, cols in COLSUM_CASES:
        x = rng_f16(rows + cols, rows, cols)
        note("colsum", {"out": oracle.colsum(x, torch.float32)}, {"out": oracle.colsum(x)})
    return worst


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def check(op, got, ref, label=""):
    for k, want in ref.items():
        err = oracle.rel_err(got[k].cpu(), want)
        print(f"{op} {label} {k}: error {err:.3e} bound {BOUNDS[op][k]:.3e}")
    for k, want in ref.items():
        assert oracle.rel_err(got[k].cpu(), want) <= BOUNDS[op][k], (op, label, k)


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int16 if a[k].dtype == torch.float16 else torch.int32),
                           b[k].view(torch.int16 if b[k].dtype == torch.float16 else torch.int32)) for k in a)


def cu_of(lens, dev):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)


def scaled(t, s):
    return (t.float() * s).half()


def properties(op, run, c, ref, grad_key, deterministic_keys=None):
    """The checks every operator gets: the oracle bound, two runs with the same bits, linearity in the incoming gradient
    (x 1024, same bound after division), and an inf gradient that returns and leaves the next call alone."""
    got = run(c)
    check(op, got, ref)
    keys = deterministic_keys if deterministic_keys is not None else list(got)
    again = run(c)
    assert same_bits({k: got[k] for k in keys}, {k: again[k] for k in keys})
    big = run(dict(c, **{grad_key: scaled(c[grad_key], 1024.0)}))
    check(op, {k: v.float() / 1024.0 for k, v in big.items()}, ref, "x1024")
    bad = c[grad_key].clone()
    bad.view(-1)[0] = float("inf")
    out = run(dict(c, **{grad_key: bad}))
    torch.cuda.synchronize()                    # returns: no fault, no endless loop
    assert any(not torch.isfinite(v).all() for v in out.values())
    after = run(c)
    assert same_bits({k: got[k] for k in keys}, {k: after[k] for k in keys})
    return got


# ---- attention ---------------------------------------------------------------------------------------------------------------

def run_attention(dev):
    from proqa_amd import trainable as T

    def run(c):
        lens = c["lens"]
        bias = None if c["bias"] is None else c["bias"].to(dev)
        d_qkv = T.attention_backward(c["qkv"].to(dev), bias, c["d_ctx"].to(dev), cu_of(lens, dev), len(lens), max(lens), c["n_heads"])
        return {"d_qkv": d_qkv}
    return run


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("n_heads,batch", ATTENTION_CASES)
def test_attention_backward(gpu_device, n_heads, batch, with_bias):
    from proqa_amd import trainable as T
    c, ref = attention_case(n_heads, batch, with_bias)
    got = properties("attention", run_attention(gpu_device), c, ref, "d_ctx")
    # the forward these gradients belong to is the inference kernel's
    ctx = T.attention(c["qkv"].to(gpu_device), None if c["bias"] is None else c["bias"].to(gpu_device), cu_of(c["lens"], gpu_device),
                      len(c["lens"]), max(c["lens"]), n_heads)
    want = oracle.attention_forward(c["qkv"].double(), None if c["bias"] is None else c["bias"].double(), c["lens"], n_heads)
    assert ((ctx.cpu().double() - want).abs() <= 4e-3 + 4e-3 * want.abs()).all()     # as tests/test_encoder_gpu.py
    # bias gradient = column sum of d_qkv; its key third is zero up to rounding
    H = 64 * n_heads
    dbias = T.colsum(got["d_qkv"]).cpu()
    assert torch.equal(dbias, T.colsum(got["d_qkv"]).cpu())
    key_third = dbias[H:2 * H].abs().max().item() / dbias.abs().max().item()
    print("key third of the bias gradient / whole:", key_third)
    assert key_third <= BOUNDS["attention"]["d_qkv"]


def test_attention_backward_near_one_hot_probabilities(gpu_device):
    c, ref = attention_case(2, "ragged", True, 6.0)
    got = run_attention(gpu_device)(c)
    assert torch.isfinite(got["d_qkv"]).all()
    print("queries x 6: error", oracle.rel_err(got["d_qkv"].cpu(), ref["d_qkv"]))       # a figure, not a bound: scores of +-150


def test_attention_backward_refuses_what_it_cannot_run(gpu_device):
    from proqa_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1024, dtype=torch.float16, device=gpu_device)
    cu = cu_of([1], gpu_device)
    ws = torch.zeros(4096, dtype=torch.uint8, device=gpu_device)
    call = lambda max_len, n_tokens, ws_bytes: lib.proqa_attention_backward_f16(
        x.data_ptr(), None, x.data_ptr(), cu.data_ptr(), 1, max_len, 2, n_tokens, x.data_ptr(), ws.data_ptr(), ws_bytes, None)
    assert call(513, 1, 4096) == -1 and call(0, 1, 4096) == -1
    assert call(1, 1, 15) == -1 and b"workspace" in lib.proqa_last_error()
    assert lib.proqa_attention_backward_workspace_bytes(300, 12) == 2 * 300 * 12 * 4


# ---- bias + residual + LayerNorm -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,magnitude", LAYERNORM_CASES)
def test_bias_residual_layernorm_backward(gpu_device, rows, cols, magnitude):
    from proqa_amd import trainable as T
    c, ref = layernorm_case(rows, cols, magnitude)

    def run(c):
        d = {k: v.to(gpu_device) for k, v in c.items() if k != "eps"}
        out = T.bias_residual_layernorm_backward(d["dy"], d["x"], d["bias"], d["residual"], d["gamma"], c["eps"])
        return dict(zip(("dz", "dgamma", "dbeta", "dbias"), out))

    got = properties("layernorm", run, c, ref, "dy")
    assert got["dz"].dtype == torch.float16 and all(got[k].dtype == torch.float32 for k in ("dgamma", "dbeta", "dbias"))


# ---- bias + GELU -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", GELU_CASES)
def test_bias_gelu_backward(gpu_device, rows, cols):
    from proqa_amd import trainable as T
    c, ref = gelu_case(rows, cols)
    t = (c["x_pre"].float() + c["bias"].float())
    assert all((t == v).any() for v in GELU_SPECIALS)

    def run(c):
        dx, dbias = T.bias_gelu_backward(c["dy"].to(gpu_device), c["x_pre"].to(gpu_device), c["bias"].to(gpu_device))
        return {"dx": dx, "dbias": dbias}

    got = properties("gelu", run, c, ref, "dy")
    assert torch.isfinite(got["dx"]).all() and torch.isfinite(got["dbias"]).all()
    # the out-of-place forward is the in-place forward kernel's expression
    y = T.bias_gelu(c["x_pre"].to(gpu_device), c["bias"].to(gpu_device)).cpu()
    finite = t.abs() < 100
    want = oracle.gelu(t.double())
    assert ((y.double() - want).abs() <= 2e-3 + 2e-3 * want.abs())[finite].all()             # as tests/test_encoder_gpu.py
    assert y[t == 6e4].eq(6e4).all() and y[t == -6e4].eq(0).all()


# ---- embedding + LayerNorm ------------------------------------------------------------------------------------------------------

def run_embed(dev):
    from proqa_amd import trainable as T

    def run(c):
        out = T.embed_layernorm_backward(c["dy"].to(dev), c["ids"].to(dev), cu_of(c["lens"], dev), c["word"].to(dev),
                                         c["pos"].to(dev), c["type0"].to(dev), c["gamma"].to(dev), c["eps"])
        return dict(zip(("dgamma", "dbeta", "d_word", "d_pos", "d_type0"), out))
    return run


@pytest.mark.parametrize("hidden,lens", EMBED_CASES)
def test_embed_layernorm_backward(gpu_device, hidden, lens):
    from proqa_amd import trainable as T
    c, ref = embed_case(hidden, lens)
    got = properties("embed", run_embed(gpu_device), c, ref, "dy", deterministic_keys=["dgamma", "dbeta", "d_pos", "d_type0"])
    assert all(v.dtype == torch.float32 for v in got.values())
    # ids past a sequence's length are ignored: their rows (ids 45 .. 49 appear nowhere else) are exactly zero, and so are
    # the position rows past the longest sequence
    assert (got["d_word"][EMBED_USED:] == 0).all() and (got["d_word"][:EMBED_USED] != 0).any()
    assert (got["d_pos"][max(lens):] == 0).all()
    # the forward these gradients belong to
    dev = gpu_device
    y = T.embed_layernorm(c["ids"].to(dev), cu_of(lens, dev), sum(lens), c["word"].to(dev), c["pos"].to(dev), c["type0"].to(dev),
                          c["gamma"].to(dev), torch.zeros(hidden, dtype=torch.float16, device=dev), c["eps"])
    want = oracle.embed_layernorm_forward(c["ids"], lens, c["word"].double(), c["pos"].double(), c["type0"].double(),
                                          c["gamma"].double(), torch.zeros(hidden, dtype=torch.float64), c["eps"])
    assert ((y.cpu().double() - want).abs() <= 2e-3 + 2e-3 * want.abs()).all()


def test_embed_scatter_of_one_token_per_id_is_exact(gpu_device):
    """One sequence whose ids are all different: the word row of a token and the position row of its place receive the
    same single fp32 value -- the bits must agree, and the type-0 gradient is their (compensated) sum in position order."""
    c, _ = embed_case(128, EMBED_CASES[0][1])
    ids = torch.randperm(EMBED_VOCAB, generator=torch.Generator().manual_seed(9))[None, :40].contiguous()
    c = dict(c, ids=ids, lens=(40,), dy=c["dy"][:40].contiguous())
    got = run_embed(gpu_device)(c)
    assert torch.equal(got["d_word"][ids[0].to(gpu_device)].view(torch.int32), got["d_pos"][:40].view(torch.int32))
    total, comp = (torch.zeros(128, dtype=torch.float32, device=gpu_device) for _ in range(2))
    for s in range(40):                         # the kernel's compensated sum, operation by operation
        y = got["d_pos"][s] - comp
        t = total + y
        comp = (t - total) - y
        total = t
    assert torch.equal(total.view(torch.int32), got["d_type0"].view(torch.int32))
    check("embed", got, oracle.embed_layernorm_backward(**c))


# ---- in-batch loss ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", LOSS_CASES)
def test_inbatch_loss_grad(gpu_device, name):
    from proqa_amd import trainable as T
    from proqa_amd.inbatch import inbatch_eval
    c, ref = loss_case(name)
    dev = gpu_device
    q, cc = c["q"].to(dev), c["c"].to(dev)
    target = None if c["target"] is None else c["target"].to(dev)
    lse = inbatch_eval(q, cc, target)["lse"]

    def run(scale):
        dq, dc = T.inbatch_loss_grad(q, cc, target, lse, torch.tensor(scale, device=dev))
        return {"dq": dq, "dc": dc}

    got = run(1.0)
    if name == "one":
        assert ref["dq"].abs().max() == 0 and ref["dc"].abs().max() == 0
        for k, other in (("dq", c["c"]), ("dc", c["q"])):
            err = got[k].float().abs().max().item() / other.float().abs().max().item()
            print(f"loss one {k}: error {err:.3e} (relative to the cancelling terms) bound {BOUNDS['loss'][k]:.3e}")
            assert err <= BOUNDS["loss"][k]
    else:
        check("loss", got, ref)
        check("loss", {k: v.float() / 1024.0 for k, v in run(1024.0).items()}, ref, "x1024")
    assert same_bits(got, run(1.0))
    bad = run(float("inf"))
    torch.cuda.synchronize()
    assert not torch.isfinite(bad["dq"]).all()
    assert same_bits(got, run(1.0))
    # the value these gradients belong to
    loss = T.inbatch_loss(q, cc, target)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert abs(loss.item() - oracle.inbatch_loss(c["q"].double(), c["c"].double(), c["target"]).item()) < 1e-3


# ---- column sum -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", COLSUM_CASES)
def test_colsum(gpu_device, rows, cols):
    from proqa_amd import trainable as T
    x = rng_f16(rows + cols, rows, cols)
    got = T.colsum(x.to(gpu_device))
    assert got.dtype == torch.float32 and got.shape == (cols,)
    check("colsum", {"out": got}, {"out": oracle.colsum(x)})
    assert torch.equal(got, T.colsum(x.to(gpu_device)))
    # integer-valued input: every partial sum is an integer below 2^24, exact in any order
    xi = torch.randint(-8, 9, (rows, cols), generator=torch.Generator().manual_seed(rows)).half()
    assert torch.equal(T.colsum(xi.to(gpu_device)).cpu(), xi.float().sum(0))
