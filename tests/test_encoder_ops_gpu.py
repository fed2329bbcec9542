"""The encoder's forward kernels (encoder_kernels.hip, attention_kernel.hip) against float64, element by element, under the
bounds derived in tests/encoder_ops_oracle.py (half an ulp of the output format + the operator's documented intermediate
rounding + GAMMA_op fp32 units, GAMMA_op = 4 x the measured error of a float32 restatement: the table is in that file and
tests/test_encoder_ops_host.py reproduces it and shows which kernel errors these bounds catch).  Every comparison covers
every valid output.  Shapes are the smallest that reach every lane pattern, tile edge and grid mapping of the kernels."""
import numpy as np
import pytest
import torch

import encoder_ops_oracle as O

pytestmark = pytest.mark.gpu
F16, F32 = 0, 1                                     # PROQA_F16 / PROQA_F32
CANARY = 7.0


@pytest.fixture(scope="module")
def lib(gpu_device):
    from proqa_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def out_with_canary(rows, cols, device, dtype=torch.float16):
    """[rows + 1, cols]: the last row is not the kernel's to write."""
    return torch.full((rows + 1, cols), CANARY, dtype=dtype, device=device)


def result(buf):
    """The kernel's rows as float64-comparable NumPy, after checking the canary row."""
    a = buf.cpu().numpy()
    assert (a[-1] == CANARY).all(), "the row after the output was written"
    return a[:-1]


def assert_within(got, ref, tol, what, where=None):
    got = O.f64(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(got - ref) / tol
    ratio = np.where(np.abs(got - ref) <= tol, ratio, np.inf)          # (a NaN is outside)
    if where is not None:
        ratio = ratio[where]
    bad = int((ratio > 1).sum())
    finite = ratio[np.isfinite(ratio)]
    print(f"{what}: worst |got - ref| / tol = {finite.max() if finite.size else 0:.3f}; {bad} of {ratio.size} outside")
    assert bad == 0, what


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


# ---- LayerNorm -----------------------------------------------------------------------------------------------------
def run_layernorm(lib, device, x, bias, res, gamma, beta, eps):
    from proqa_amd import _lib
    rows, cols = x.shape
    t = [dev(a, device) for a in (x, bias, res, gamma, beta)]
    out = out_with_canary(rows, cols, device)
    _lib.check(lib.proqa_bias_residual_layernorm_f16(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                                     t[4].data_ptr(), eps, rows, cols, out.data_ptr(), stream()))
    return result(out)


@pytest.mark.parametrize("cols", O.LN_COLS)
def test_bias_residual_layernorm(lib, gpu_device, cols):
    for rows in O.LN_ROWS:
        for family in O.LN_FAMILIES:
            x, bias, res, gamma, beta, eps = O.layernorm_case(cols, rows, family)
            ref = O.LayerNormRef((x, bias, res), gamma, beta, eps)
            got = run_layernorm(lib, gpu_device, x, bias, res, gamma, beta, eps)
            assert_within(got, ref.out, ref.bound(), f"layernorm {cols} x {rows} {family}")
        x, bias, res, gamma, beta = O.constant_rows_case(cols, rows)
        got = run_layernorm(lib, gpu_device, x, bias, res, gamma, beta, 1e-12)
        assert (bits(got) == bits(np.broadcast_to(beta, got.shape))).all(), "a constant row is beta bit for bit"


@pytest.mark.parametrize("cols", [1032, 12, 4, 0])
def test_layernorm_refuses_what_it_cannot_hold(lib, gpu_device, cols):
    n = max(cols, 8)
    t = torch.ones((2, n), dtype=torch.float16, device=gpu_device)
    v = torch.ones(n, dtype=torch.float16, device=gpu_device)
    out = torch.full((2, n), CANARY, dtype=torch.float16, device=gpu_device)
    assert lib.proqa_bias_residual_layernorm_f16(t.data_ptr(), v.data_ptr(), t.data_ptr(), v.data_ptr(), v.data_ptr(), 1e-12,
                                                 2, cols, out.data_ptr(), stream()) != 0
    ids = torch.zeros(2, dtype=torch.int64, device=gpu_device)
    assert lib.proqa_embed_layernorm_f16(ids.data_ptr(), 2, 2, cols, t.data_ptr(), 2, t.data_ptr(), v.data_ptr(), v.data_ptr(),
                                         v.data_ptr(), 1e-12, out.data_ptr(), stream()) != 0
    torch.cuda.synchronize()
    assert (out == CANARY).all()


@pytest.mark.parametrize("hidden,batch,seq_len", O.EMBED_CASES)
def test_embedding_layernorm_plain_typed_and_packed(lib, gpu_device, hidden, batch, seq_len):
    from proqa_amd import _lib
    c = O.embed_case(hidden, batch, seq_len)
    n_tokens = batch * seq_len
    assert n_tokens % 4
    t = {k: dev(v, gpu_device) for k, v in c.items()}
    cu_host = np.concatenate([[0], np.cumsum(c["lens"])]).astype(np.int32)
    cu, total = dev(cu_host, gpu_device), int(cu_host[-1])
    rows = O.packed_rows(c["lens"], seq_len)
    p = lambda k: t[k].data_ptr()
    for typed in (False, True):
        ref = O.LayerNormRef(O.embed_parts(c, typed), c["gamma"], c["beta"], 1e-12)
        tol = ref.bound()
        out = out_with_canary(n_tokens, hidden, gpu_device)
        packed = out_with_canary(total, hidden, gpu_device)
        if typed:
            _lib.check(lib.proqa_embed_layernorm_typed_f16(p("ids"), p("type_ids"), n_tokens, seq_len, hidden, p("word"),
                                                           O.EMBED_VOCAB, p("pos"), p("types"), O.EMBED_TYPES, p("gamma"),
                                                           p("beta"), 1e-12, out.data_ptr(), stream()))
            _lib.check(lib.proqa_embed_layernorm_typed_varlen_f16(p("ids"), p("type_ids"), cu.data_ptr(), batch, seq_len, hidden,
                                                                  p("word"), O.EMBED_VOCAB, p("pos"), p("types"), O.EMBED_TYPES,
                                                                  p("gamma"), p("beta"), 1e-12, packed.data_ptr(), stream()))
        else:
            _lib.check(lib.proqa_embed_layernorm_f16(p("ids"), n_tokens, seq_len, hidden, p("word"), O.EMBED_VOCAB, p("pos"),
                                                     p("types"), p("gamma"), p("beta"), 1e-12, out.data_ptr(), stream()))
            _lib.check(lib.proqa_embed_layernorm_varlen_f16(p("ids"), cu.data_ptr(), batch, seq_len, hidden, p("word"),
                                                            O.EMBED_VOCAB, p("pos"), p("types"), p("gamma"), p("beta"), 1e-12,
                                                            packed.data_ptr(), stream()))
        got, got_packed = result(out), result(packed)
        assert_within(got, ref.out, tol, f"embedding {hidden} typed={typed}")
        assert (bits(got_packed) == bits(got[rows])).all(), "the packed rows are the padded evaluation's valid rows"


# ---- GELU ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,x,bias", list(O.gelu_cases()), ids=["bias0", "mixed"])
def test_bias_gelu_every_finite_fp16(lib, gpu_device, name, x, bias):
    from proqa_amd import _lib
    rows, cols = x.shape
    tx, tb = dev(x, gpu_device), dev(bias, gpu_device)
    out = out_with_canary(rows, cols, gpu_device)
    _lib.check(lib.proqa_bias_gelu_out_f16(tx.data_ptr(), tb.data_ptr(), rows, cols, out.data_ptr(), stream()))
    inplace = torch.cat([tx, torch.full((1, cols), CANARY, dtype=torch.float16, device=gpu_device)])
    _lib.check(lib.proqa_bias_gelu_f16(inplace.data_ptr(), tb.data_ptr(), rows, cols, stream()))
    got, got_inplace = result(out), result(inplace)
    assert (bits(got) == bits(got_inplace)).all(), "in place and out of place agree bit for bit"
    bad = O.gelu_mismatches(got, x, bias)
    print(f"gelu {name}: {int(bad.sum())} of {bad.size} outside; first: x = {x[bad][:4]}, got {got[bad][:4]}")
    assert not bad.any()


# ---- attention -----------------------------------------------------------------------------------------------------
def run_attention(lib, device, qkv, bias, lens, NH, layout, cls_only):
    """proqa_attention_ex_f16 -> [B, Sq, H] float64 with NaN where the layout has no row; status when it refuses."""
    B, S = qkv.shape[:2]
    H = NH * O.HEAD
    lens_c = O.clamp_lens(lens, S)
    flat = np.asarray(qkv).reshape(B * S, 3 * H)
    tb = None if bias is None else dev(bias, device)
    bp = None if bias is None else tb.data_ptr()
    if layout == "padded":
        tq, tl = dev(flat, device), dev(np.asarray(lens, dtype=np.int32), device)
        out = out_with_canary(B if cls_only else B * S, H, device)
        status = lib.proqa_attention_ex_f16(tq.data_ptr(), bp, tl.data_ptr(), None, B, S, NH, int(cls_only), out.data_ptr(), stream())
        if status:
            return status
        return O.f64(result(out)).reshape(B, -1, H)
    rows = O.packed_rows(lens_c, S)
    tq = dev(flat[rows], device)
    cu = dev(np.concatenate([[0], np.cumsum(lens_c)]).astype(np.int32), device)
    out = out_with_canary(B if cls_only else len(rows), H, device)
    status = lib.proqa_attention_ex_f16(tq.data_ptr(), bp, None, cu.data_ptr(), B, int(lens_c.max()), NH, int(cls_only),
                                        out.data_ptr(), stream())
    if status:
        return status
    got = O.f64(result(out))
    if cls_only:
        return got.reshape(B, 1, H)
    full = np.full((B * S, H), np.nan)
    full[rows] = got
    return full.reshape(B, S, H)


ATTENTION_CASES = O.attention_cases()


@pytest.mark.parametrize("case", ATTENTION_CASES, ids=[c["name"] for c in ATTENTION_CASES])
def test_attention_both_layouts_full_and_cls(lib, gpu_device, case):
    qkv, bias = O.attention_case_inputs(case)
    ref = O.AttentionRef(qkv, bias, case["lens"], case["NH"])
    out, tol, valid = ref.out, ref.bound(), ref.valid()
    for layout in ("padded", "packed"):
        got = run_attention(lib, gpu_device, qkv, bias, case["lens"], case["NH"], layout, False)
        assert_within(got, out, tol, f"attention {case['name']} {layout}", valid)
        got = run_attention(lib, gpu_device, qkv, bias, case["lens"], case["NH"], layout, True)
        assert_within(got, out[:, :1], ref.bound_cls(), f"attention [CLS] {case['name']} {layout}")
    if case["name"] == "key_bias40":                 # the key bias is mathematically absent: the reference never saw it (the
        #                                              [CLS] kernel's bound carries the fp16 rounding of k + 40: bound_cls())
        assert (np.asarray(bias)[128:256] == 40).all()
    if case["name"].startswith("zero_q"):            # q = 0 (and b_q = 0): the mean of V over the valid keys (+ b_v)
        v = O.f64(qkv).reshape(case["B"], case["S"], 3, case["NH"], 64)[:, :, 2]
        for b, n in enumerate(ref.lens):
            mean = v[b, :n].mean(0).reshape(-1) + (0 if bias is None else O.f64(bias)[2 * case["NH"] * 64:])
            np.testing.assert_allclose(out[b, :n], np.broadcast_to(mean, (n, mean.size)), rtol=1e-12, atol=1e-14)


def test_attention_lengths_outside_the_range_are_clamped(lib, gpu_device):
    S, lens = 40, (0, 45, 5)
    qkv, bias = O.attention_inputs("clamped", 3, S, 1, lens, with_bias=True)
    ref = O.AttentionRef(qkv, bias, lens, 1)
    assert list(ref.lens) == [1, 40, 5]
    for cls_only in (False, True):
        got = run_attention(lib, gpu_device, qkv, bias, lens, 1, "padded", cls_only)
        n = 1 if cls_only else S
        tol = ref.bound_cls() if cls_only else ref.bound()
        assert_within(got, ref.out[:, :n], tol, f"lens 0 and S + 5, cls={cls_only}", ref.valid()[:, :n])


def test_attention_cls_sequence_length_limit(lib, gpu_device):
    lens = (4096, 3001)
    qkv, bias = O.attention_inputs("cls4096", 2, 4096, 1, lens, with_bias=True)
    ref = O.AttentionRef(qkv, bias, lens, 1, cls_only=True)
    for layout in ("padded", "packed"):
        got = run_attention(lib, gpu_device, qkv, bias, lens, 1, layout, True)
        assert_within(got, ref.out, ref.bound_cls(), f"[CLS] S = 4096 {layout}")
    longer = np.zeros((1, 4097, 192), np.float16)
    assert run_attention(lib, gpu_device, longer, None, (4097,), 1, "padded", True) != 0
    assert run_attention(lib, gpu_device, longer, None, (4097,), 1, "packed", True) != 0


@pytest.mark.parametrize("fill", ["huge", "nonfinite"])
def test_attention_padding_rows_never_reach_a_valid_query(lib, gpu_device, fill):
    """Padded layout: whatever the K and V of the rows >= len hold, the valid queries' outputs are those of the zero-filled
    run, bit for bit -- in the full kernel (whose last key tile holds masked keys with probability exactly 0) and in the
    [CLS] kernel.  Before attention_fwd staged K / V for the valid keys only (it staged every row of the sequence), the
    NaN / Inf fill made 90368 of the 217472 valid outputs of the full kernel NaN (0 x NaN in P V); the finite fill made none
    differ, and the [CLS] kernel, which skips masked keys, was clean."""
    NH, S = 2, 257
    H = NH * 64
    qkv, bias = O.attention_inputs("padding", 16, S, NH, O.EDGE_LENS, with_bias=True)
    x = np.array(qkv).reshape(16, S, 3, H)
    pad = np.arange(S)[None, :] >= np.asarray(O.EDGE_LENS)[:, None]
    r = np.random.default_rng(5)
    if fill == "huge":
        values = np.array([60000.0, -60000.0, 65504.0, -65504.0], np.float16)
    else:
        values = np.array([np.nan, np.inf, -np.inf, np.nan], np.float16)
    zeroed, filled = x.copy(), x.copy()
    zeroed[:, :, 1:][pad] = 0
    filled[:, :, 1:][pad] = values[r.integers(0, 4, (int(pad.sum()), 2, H))]
    ref = O.AttentionRef(zeroed.reshape(16, S, 3 * H), bias, O.EDGE_LENS, NH)
    valid = ref.valid()
    for cls_only in (False, True):
        a = run_attention(lib, gpu_device, zeroed.reshape(16, S, 3 * H), bias, O.EDGE_LENS, NH, "padded", cls_only)
        b = run_attention(lib, gpu_device, filled.reshape(16, S, 3 * H), bias, O.EDGE_LENS, NH, "padded", cls_only)
        v = valid[:, :a.shape[1]]
        differ = ~((a == b) | (np.isnan(a) & np.isnan(b)))[v]
        print(f"padding fill {fill}, cls={cls_only}: {int(differ.sum())} of {differ.size} valid outputs differ from the "
              f"zero-filled run, {int(np.isnan(b[v]).sum())} are NaN")
        assert not differ.any()
        assert_within(a, ref.out[:, :a.shape[1]], ref.bound_cls() if cls_only else ref.bound(), f"zero-filled padding, cls={cls_only}", v)


# ---- pooler + projection ---------------------------------------------------------------------------------------------
def run_pool_project(lib, device, h, wp, bp, wj, bj, out_dtype):
    from proqa_amd import _lib
    B, S, hidden = h.shape
    t = [dev(a, device) for a in (h, wp, bp, wj, bj)]
    ws = torch.empty((B, hidden), dtype=torch.float16, device=device)
    out = out_with_canary(B, O.EMBED_DIM, device, torch.float32 if out_dtype == F32 else torch.float16)
    _lib.check(lib.proqa_pool_project_f16(t[0].data_ptr(), B, S, hidden, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                          t[4].data_ptr(), ws.data_ptr(), out.data_ptr(), out_dtype, stream()))
    return result(out)


@pytest.mark.parametrize("hidden", O.POOL_HIDDEN)
def test_pool_project(lib, gpu_device, hidden):
    for batch in O.POOL_BATCH:
        for saturate in (False, True):
            args = O.pooler_inputs(hidden, batch, saturate=saturate)
            ref = O.PoolerRef(*args)
            for out_dtype in (F16, F32):
                got = run_pool_project(lib, gpu_device, *args, out_dtype)
                assert_within(got, ref.out, ref.bound(out32=out_dtype == F32),
                              f"pool_project {hidden} x {batch} saturate={saturate} out={out_dtype}")
        args, expect = O.pooler_integer_inputs(hidden, batch)
        assert np.abs(expect).max() <= 2048
        assert (O.f64(run_pool_project(lib, gpu_device, *args, F32)) == expect).all(), "tanh(+-32) = +-1, integer projection"
        assert (O.f64(run_pool_project(lib, gpu_device, *args, F16)) == expect).all()


# ---- small dense layer -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoder_handle(gpu_device):
    from proqa_amd.retriever import BertForRetriever, random_state_dict, BERT_BASE
    cfg = dict(BERT_BASE, num_hidden_layers=1)
    model = BertForRetriever(cfg, device=gpu_device)
    model.load_state_dict(random_state_dict(cfg, seed=0))
    yield model.towers[False]._handle
    del model


def run_dense(lib, device, handle, x, w, bias, act):
    """handle: proqa_encoder_dense (no bias, no activation); None: proqa_small_dense_f16."""
    from proqa_amd import _lib
    M, K = x.shape
    N = w.shape[0]
    tx, tw = dev(x, device), dev(w, device)
    tb = None if bias is None else dev(bias, device)
    out = out_with_canary(M, N, device)
    if handle is not None:
        _lib.check(lib.proqa_encoder_dense(handle, tx.data_ptr(), tw.data_ptr(), out.data_ptr(), M, N, K, stream()))
    else:
        _lib.check(lib.proqa_small_dense_f16(tx.data_ptr(), M, tw.data_ptr(), None if tb is None else tb.data_ptr(), N, K, act,
                                             out.data_ptr(), stream()))
    return result(out)


@pytest.mark.parametrize("M", O.DENSE_M)
def test_small_dense_layer(lib, gpu_device, encoder_handle, M):
    for N in O.DENSE_N:
        for K in O.DENSE_K:
            xi, wi, bi = O.dense_inputs(M, N, K, "int")
            x, w, bias = O.dense_inputs(M, N, K, "gauss")
            exact, exact_b = O.DenseRef(xi, wi), O.DenseRef(xi, wi, bi)
            assert np.abs(exact_b.out).max() <= 2048
            plain, biased, gelu = O.DenseRef(x, w), O.DenseRef(x, w, bias), O.DenseRef(x, w, bias, act=1)
            what = f"dense {M} x {N} x {K}"
            assert (O.f64(run_dense(lib, gpu_device, encoder_handle, xi, wi, None, 0)) == exact.out).all(), what
            assert_within(run_dense(lib, gpu_device, encoder_handle, x, w, None, 0), plain.out, plain.bound(), what + " encoder_dense")
            assert (O.f64(run_dense(lib, gpu_device, None, xi, wi, None, 0)) == exact.out).all(), what
            assert (O.f64(run_dense(lib, gpu_device, None, xi, wi, bi, 0)) == exact_b.out).all(), what
            assert_within(run_dense(lib, gpu_device, None, x, w, bias, 0), biased.out, biased.bound(), what + " bias")
            assert_within(run_dense(lib, gpu_device, None, x, w, bias, 1), gelu.out, gelu.bound(), what + " bias + gelu")


@pytest.mark.parametrize("n_feat,k,act", [(48, 128, 0), (32, 192, 0), (32, 64, 1), (0, 128, 0), (32, 0, 0), (32, 128, 2)])
def test_small_dense_refuses_other_shapes(lib, gpu_device, n_feat, k, act):
    x = torch.ones((4, 256), dtype=torch.float16, device=gpu_device)
    w = torch.ones((64, 256), dtype=torch.float16, device=gpu_device)
    out = torch.full((4, 64), CANARY, dtype=torch.float16, device=gpu_device)
    assert lib.proqa_small_dense_f16(x.data_ptr(), 4, w.data_ptr(), None, n_feat, k, act, out.data_ptr(), stream()) != 0
    torch.cuda.synchronize()
    assert (out == CANARY).all()
    assert lib.proqa_small_dense_f16(x.data_ptr(), 0, w.data_ptr(), None, n_feat, k, act, out.data_ptr(), stream()) != 0
    assert lib.proqa_small_dense_f16(x.data_ptr(), 0, w.data_ptr(), None, 32, 128, 0, out.data_ptr(), stream()) == 0
