"""proqa_embed_layernorm_typed_varlen_backward_f16 (csrc/train_kernels.hip) against tests/reader_train_oracle.py: the closed
form of the embedding + LayerNorm backward with token types, in float64 on the kernel's own fp16 inputs.

Error measure, per output tensor: max|gpu - ref| / max|ref|, the incoming gradient at loss scale 1024.

Tolerance: four times the same measure of the oracle's storage="fp16" mode (fp32 arithmetic; every output of this operator
is an fp32 parameter gradient, so nothing is rounded to fp16) against float64, the maximum over the cases below --
measure_reference_error(), run on the CPU (tests/test_trainable_reader_host.py reproduces the table).  The factor 4 is what
this project gives device intrinsics and re-associated sums over libm (tests/test_train_ops_gpu.py).  Measured
(REFERENCE_ERROR) and allowed (BOUNDS):

    output     measured    bound
    dgamma     2.015e-07   8.060e-07
    dbeta      6.028e-08   2.411e-07
    d_word     2.124e-07   8.496e-07
    d_pos      1.691e-07   6.764e-07
    d_types    1.118e-06   4.472e-06

Shapes (hidden, batch, seq_len): hidden 128 leaves lanes without a chunk, 768 fills the second chunk of a lane partly, 1024
fills it; batch 5 and 9 give a wave a second and third turn; (128, 1, 1) is one token; seq_len 512 is the slab limit.
Id patterns: segments 0 then 1, all 0, all 1, ids outside their tables (type 7 and -1, a word id past the vocabulary: row 0
of the table in the forward, and here), and a one-row type table.
"""
import functools

import numpy as np
import pytest
import torch

import reader_train_oracle as oracle

pytestmark = pytest.mark.gpu

REFERENCE_ERROR = {"dgamma": 2.015e-07, "dbeta": 6.028e-08, "d_word": 2.124e-07, "d_pos": 1.691e-07, "d_types": 1.118e-06}
BOUNDS = {k: 4.0 * v for k, v in REFERENCE_ERROR.items()}
OUTPUTS = ("dgamma", "dbeta", "d_word", "d_pos", "d_types")
DETERMINISTIC = ("dgamma", "dbeta", "d_pos", "d_types")
LOSS_SCALE = 1024.0
VOCAB, EXTRA_POSITIONS = 50, 3

# (hidden, lens): batch = len(lens), seq_len = max(lens); ragged, a length of 1 wherever the batch has room for one
SHAPES = {
    (128, 5, 40): (40, 33, 1, 9, 27),
    (768, 5, 24): (17, 24, 1, 5, 24),
    (1024, 3, 16): (16, 1, 11),
    (128, 1, 1): (1,),
    (128, 9, 12): (12, 1, 7, 12, 3, 9, 10, 2, 5),
    (128, 2, 512): (512, 1),
}
PATTERNS = ("segments", "all0", "all1", "outside", "one_type")


def rng_f16(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).half()


@functools.lru_cache(maxsize=None)
def case(shape, pattern):
    """CPU tensors of one case and its float64 reference, computed once"""
    hidden, batch, seq_len = shape
    lens = SHAPES[shape]
    assert len(lens) == batch and max(lens) == seq_len
    seed = hidden + 7 * batch + seq_len
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, VOCAB, (batch, seq_len), generator=g)
    ar = torch.arange(seq_len)[None]
    question = torch.tensor([max(1, n // 3) for n in lens])[:, None]
    n_types = 1 if pattern == "one_type" else 2
    if pattern in ("segments", "one_type"):          # (one_type: the ids say 0 / 1, the table has row 0 only)
        type_ids = (ar >= question).long().expand(batch, seq_len).contiguous()
    elif pattern == "all0":
        type_ids = torch.zeros((batch, seq_len), dtype=torch.int64)
    elif pattern == "all1":
        type_ids = torch.ones((batch, seq_len), dtype=torch.int64)
    else:
        type_ids = (ar >= question).long().expand(batch, seq_len).contiguous()
        type_ids[:, 0] = 7                              # every sequence has a token 0
        type_ids[0, seq_len - 1] = -1                   # sequence 0 is (one of) the longest
        ids[0, 0] = VOCAB + 5
        ids[batch - 1, 0] = -3
    c = dict(dy=(rng_f16(seed + 1, sum(lens), hidden).float() * LOSS_SCALE).half(), ids=ids, type_ids=type_ids, lens=lens,
             word=rng_f16(seed + 2, VOCAB, hidden), pos=rng_f16(seed + 3, seq_len + EXTRA_POSITIONS, hidden),
             types=rng_f16(seed + 4, n_types, hidden), gamma=(1.0 + 0.1 * torch.randn(hidden, generator=g)).half(), eps=1e-12)
    assert torch.isfinite(c["dy"]).all()
    return c, oracle.embed_typed_backward(**c)


def measure_reference_error():
    """{output: max over the cases of rel_err(storage='fp16' oracle, float64 oracle)} -- CPU only; the table in the header
    and REFERENCE_ERROR are its output."""
    worst = {}
    for shape in SHAPES:
        for pattern in PATTERNS:
            c, ref = case(shape, pattern)
            got = oracle.embed_typed_backward(**c, dtype=torch.float32, storage="fp16")
            for k in OUTPUTS:
                worst[k] = max(worst.get(k, 0.0), oracle.rel_err(got[k], ref[k]))
    return worst


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def cu_of(lens, dev):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)


def bits(t):
    return t.view(torch.int32)


def run(dev, c, typed=True):
    from proqa_amd import trainable as T
    out = T.embed_layernorm_typed_backward(c["dy"].to(dev), c["ids"].to(dev), c["type_ids"].to(dev) if typed else None,
                                           cu_of(c["lens"], dev), c["word"].to(dev), c["pos"].to(dev), c["types"].to(dev),
                                           c["gamma"].to(dev), c["eps"])
    return dict(zip(OUTPUTS, out))


def check(got, ref, label=""):
    errors = {k: oracle.rel_err(got[k].cpu(), ref[k]) for k in OUTPUTS}
    for k in OUTPUTS:
        print(f"{label} {k}: error {errors[k]:.3e} bound {BOUNDS[k]:.3e}")
    for k in OUTPUTS:
        assert errors[k] <= BOUNDS[k], (label, k, errors[k], BOUNDS[k])


def raw_call(dev, c, *, fill=0.0, n_types=None, hidden=None, seq_len=None, ws_bytes=None):
    """The entry point itself over buffers filled with `fill` -> (status, outputs)"""
    from proqa_amd import _lib
    lib = _lib.load()
    d = {k: v.to(dev) for k, v in c.items() if torch.is_tensor(v)}
    batch, S = c["ids"].shape
    H = c["word"].shape[1]
    out = {"dgamma": torch.full((H,), fill, device=dev), "dbeta": torch.full((H,), fill, device=dev),
           "d_word": torch.full(c["word"].shape, fill, device=dev), "d_pos": torch.full(c["pos"].shape, fill, device=dev),
           "d_types": torch.full(c["types"].shape, fill, device=dev)}
    need = lib.proqa_embed_layernorm_typed_backward_workspace_bytes(H)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        status = lib.proqa_embed_layernorm_typed_varlen_backward_f16(
            d["dy"].data_ptr(), d["ids"].data_ptr(), d["type_ids"].data_ptr(), cu_of(c["lens"], dev).data_ptr(), batch,
            S if seq_len is None else seq_len, H if hidden is None else hidden, sum(c["lens"]), d["word"].data_ptr(), VOCAB,
            d["pos"].data_ptr(), d["types"].data_ptr(), c["types"].shape[0] if n_types is None else n_types, d["gamma"].data_ptr(),
            c["eps"], out["dgamma"].data_ptr(), out["dbeta"].data_ptr(), out["d_word"].data_ptr(), out["d_pos"].data_ptr(),
            out["d_types"].data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes, _lib.current_stream_ptr())
    torch.cuda.synchronize(dev)
    return status, out


# ---- the tests -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_typed_backward_matches_float64(gpu_device, shape, pattern):
    c, ref = case(shape, pattern)
    got = run(gpu_device, c)
    assert all(got[k].dtype == torch.float32 and got[k].shape == ref[k].shape for k in OUTPUTS)
    check(got, ref, f"{shape} {pattern}")
    lens = c["lens"]
    assert (got["d_pos"][max(lens):] == 0).all()                      # rows past the longest sequence stay untouched
    if pattern == "all0":
        assert (got["d_types"][1] == 0).all() and (got["d_types"][0] != 0).any()       # exactly 0.0
    if pattern == "all1":
        assert (got["d_types"][0] == 0).all() and (got["d_types"][1] != 0).any()
    if pattern == "one_type":
        assert got["d_types"].shape == (1, shape[0])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_two_runs_scaling_and_accumulation(gpu_device, shape):
    c, ref = case(shape, "segments")
    got, again = run(gpu_device, c), run(gpu_device, c)
    for k in DETERMINISTIC:
        assert torch.equal(bits(got[k]), bits(again[k])), k
    # linear in dy: a power of two scales every deterministic output exactly; d_word (atomics) within the bound
    for factor in (2.0 ** -3, 2.0 ** 2):              # (dy is at loss scale 1024 already: 2^4 more would overflow fp16)
        dy = (c["dy"].float() * factor).half()
        assert torch.isfinite(dy).all() and torch.equal(dy.float(), c["dy"].float() * factor)
        scaled = run(gpu_device, dict(c, dy=dy))
        for k in DETERMINISTIC:
            assert torch.equal(bits(scaled[k]), bits(got[k] * factor)), (k, factor)
        check({k: v / factor for k, v in scaled.items()}, ref, f"{shape} x{factor}")
    # added into, not overwritten
    status, filled = raw_call(gpu_device, c, fill=3.0)
    assert status == 0
    for k in DETERMINISTIC:
        want = got[k] + 3.0
        if k == "d_pos":
            want[max(c["lens"]):] = 3.0
        assert torch.equal(bits(filled[k]), bits(want)), k
    check(dict(filled, d_word=filled["d_word"] - 3.0, **{k: got[k] for k in DETERMINISTIC}), ref, f"{shape} filled")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_null_type_ids_is_the_untyped_operator(gpu_device, shape):
    from proqa_amd import trainable as T
    c, _ = case(shape, "segments")
    dev = gpu_device
    got = run(dev, c, typed=False)
    untyped = dict(zip(("dgamma", "dbeta", "d_word", "d_pos", "d_type0"), T.embed_layernorm_backward(
        c["dy"].to(dev), c["ids"].to(dev), cu_of(c["lens"], dev), c["word"].to(dev), c["pos"].to(dev),
        c["types"][0].contiguous().to(dev), c["gamma"].to(dev), c["eps"])))
    for k in ("dgamma", "dbeta", "d_pos"):
        assert torch.equal(bits(got[k]), bits(untyped[k])), k
    ref = oracle.embed_typed_backward(**dict(c, type_ids=None))
    check(got, ref, f"{shape} NULL")
    assert oracle.rel_err(got["d_types"][0].cpu(), untyped["d_type0"].cpu()) <= BOUNDS["d_types"]
    assert (got["d_types"][1] == 0).all()


def test_nan_reaches_the_type_gradient_and_one_position(gpu_device):
    c, _ = case((128, 5, 40), "segments")
    lens = c["lens"]
    dy = c["dy"].clone()
    b, s = 1, 3                                            # token (1, 3): type 0 (the question part of 33 tokens is 11 long)
    dy[lens[0] + s] = float("nan")
    got = run(gpu_device, dict(c, dy=dy))
    assert not torch.isfinite(got["d_types"][0]).any() and torch.isfinite(got["d_types"][1]).all()
    assert not torch.isfinite(got["d_pos"][s]).any()
    others = torch.ones(got["d_pos"].shape[0], dtype=torch.bool)
    others[s] = False
    assert torch.isfinite(got["d_pos"][others.to(gpu_device)]).all()
    clean = run(gpu_device, c)                             # and the next call is untouched
    assert all(torch.isfinite(clean[k]).all() for k in OUTPUTS)


def test_refuses_what_it_cannot_run(gpu_device):
    from proqa_amd import _lib
    lib = _lib.load()
    c, _ = case((128, 5, 40), "segments")
    assert lib.proqa_embed_layernorm_typed_backward_workspace_bytes(128) == 512 * 4 * 128 * 4
    assert lib.proqa_backward_workspace_bytes(128) == 512 * 3 * 128 * 4              # unchanged
    for kw, word in ((dict(n_types=3), b"n_types"), (dict(n_types=0), b"n_types"), (dict(hidden=100), b"hidden"),
                     (dict(seq_len=513), b"seq_len"), (dict(ws_bytes=lib.proqa_backward_workspace_bytes(128)), b"workspace")):
        status, out = raw_call(gpu_device, c, fill=7.0, **kw)
        assert status == -1 and word in lib.proqa_last_error(), (kw, lib.proqa_last_error())
        assert all((v == 7.0).all() for v in out.values()), kw


def test_forward_and_backward_under_autograd(gpu_device):
    from proqa_amd.trainable import _EmbedLayerNormTyped
    dev = gpu_device
    c, ref = case((128, 5, 40), "segments")
    lens = c["lens"]
    params = [c[k].float().to(dev).requires_grad_(True) for k in ("word", "pos", "types", "gamma")]
    beta = torch.zeros(128, device=dev, requires_grad=True)
    y = _EmbedLayerNormTyped.apply(c["ids"].to(dev), c["type_ids"].to(dev), cu_of(lens, dev), sum(lens), *params, beta, c["eps"])
    want = oracle.embed_typed_forward(c["ids"], c["type_ids"], lens, c["word"].double(), c["pos"].double(), c["types"].double(),
                                      c["gamma"].double(), torch.zeros(128, dtype=torch.float64), c["eps"])
    assert y.dtype == torch.float16 and ((y.detach().cpu().double() - want).abs() <= 2e-3 + 2e-3 * want.abs()).all()
    y.backward(c["dy"].to(dev))
    d_types = params[2].grad
    assert d_types.shape == (2, 128) and d_types.dtype == torch.float32 and (d_types[0] != 0).any() and (d_types[1] != 0).any()
    direct = run(dev, c)
    assert torch.equal(bits(d_types), bits(direct["d_types"])) and torch.equal(bits(beta.grad), bits(direct["dbeta"]))
    check({"dgamma": params[3].grad, "dbeta": beta.grad, "d_word": params[0].grad, "d_pos": params[1].grad, "d_types": d_types},
          ref, "autograd")
