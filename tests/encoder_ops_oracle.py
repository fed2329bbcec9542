"""Float64 references, derived bounds and the shared case lists of the encoder's forward operators
(encoder_kernels.hip, attention_kernel.hip): LayerNorm, erf-GELU, masked attention with the folded Q|K|V bias, the pooler
+ projection and the small dense layer.  NumPy / torch-CPU only: tests/test_encoder_ops_host.py runs it without a GPU,
tests/test_encoder_ops_gpu.py holds the kernels to it.

BOUNDS.  Every operator is compared element by element with a float64 evaluation of the same operation on the same fp16
operands, under

    tol = ulp(|ref| + t) / 2  +  t,      t = (the operator's documented intermediate rounding) + GAMMA_op x unit_op

ulp is the fp16 spacing (fp32 for an fp32 output): the final rounding of a value that is within t of ref.  unit_op is the
size of one fp32 rounding of the operator's own sums (below, per operator); GAMMA_op is MEASURED, never fitted to a kernel:
measure_reference_error() evaluates a plain float32 restatement of the operation (the *_f32 functions here, NumPy sums in
NumPy's order) against float64 on the very case lists the GPU tests use, takes the largest |f32 - f64| / unit_op over every
element of every case, and GAMMA_op = 4 x that.  The factor 4 is what the restatement does not share with the kernel: the
tree order of the wave sums, rsqrtf / v_exp_f32 / the device erff and tanhf being a couple of ulps off, and the MFMA
accumulation order.  A kernel that misses a bound is a finding to explain, not a constant to raise.

MEASURED (python tests/encoder_ops_oracle.py prints the table; tests/test_encoder_ops_host.py reproduces it):

    operator    unit_op                                                        worst ratio    GAMMA = 4 x
    layernorm   2^-24 (|g_i| (max|x_row| / sigma_row + |xhat_i|) + |ref_i|)    %(layernorm)s
    gelu        2^-24 |t| (1 + |t|)     (absolute: 1 + erf cancels for t << 0)   %(gelu)s
    attention   2^-24 (sum_j p_j |v_j|) (1 + max_j |s_j|)                       %(attention)s
    dense       2^-24 (sum_k |x_k| |w_k| + |bias|)                              %(dense)s
    pooler      the dense unit through tanh' <= 1, see PoolerRef.unit()        %(pooler)s

Documented intermediate roundings: attention rounds the probabilities to fp16 before P V (2^-11 sum_j p_j |v_j|, and
2^-25 |v_j| / l for a probability in fp16's subnormal range), and with a bias rounds the context to fp16 before the value
bias is added in fp16; the pooler stores tanh(.) as fp16 between its two products; GELU after the small dense layer acts on
the fp32 sum (no rounding between them).
"""
import math
import zlib

import numpy as np
import torch

# measure_reference_error() on the CPU: worst |float32 restatement - float64| / unit over the case lists below
REFERENCE_RATIO = {
    "layernorm": 3.0706,      # GAMMA = 12.2824
    "gelu": 1.1128,           # GAMMA = 4.4512
    "attention": 5.1569,      # GAMMA = 20.6276
    "dense": 5.2585,          # GAMMA = 21.034
    "pooler": 0.3587,         # GAMMA = 1.4348
}
GAMMA = {op: 4.0 * r for op, r in REFERENCE_RATIO.items()}
__doc__ = __doc__ % {op: f"{r:8.3f}     {4 * r:8.3f}" for op, r in REFERENCE_RATIO.items()}

U24 = 2.0 ** -24


def f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def ulp16(x):
    """Spacing of fp16 at |x| (2^-24 in the subnormal range; the top binade's above 65504)."""
    e = np.floor(np.log2(np.maximum(np.abs(f64(x)), 2.0 ** -14)))
    return 2.0 ** (np.minimum(e, 15.0) - 10.0)


def ulp32(x):
    e = np.floor(np.log2(np.maximum(np.abs(f64(x)), 2.0 ** -126)))
    return 2.0 ** (e - 23.0)


def final_rounding(ref, t, out32=False):
    """Half a spacing of the output format at a value within t of ref."""
    return (ulp32 if out32 else ulp16)(np.abs(ref) + t) / 2


def rng_of(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def h16(a):
    return np.asarray(a).astype(np.float16)


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm(x + bias + residual) and the embedding LayerNorm (the same row operator on word + pos + type)
# ------------------------------------------------------------------------------------------------------------------
LN_COLS = (8, 504, 512, 520, 768, 1016, 1024)      # 1, 63, 64, 65, 96, 127, 128 sixteen-byte chunks per row
LN_ROWS = (1, 3, 4, 5, 9)                          # both sides of the 4-row block
LN_FAMILIES = ("normal", "mean30", "tiny_eps1e-12", "tiny_eps1e-5", "scale100")


class LayerNormRef:
    def __init__(self, parts, gamma, beta, eps):
        """parts: the fp16 operands whose sum is normalised (each [rows, cols] or broadcastable)."""
        x = sum(f64(p) for p in parts)               # exact: a few fp16 values in float64
        self.gamma, self.beta = f64(gamma), f64(beta)
        mean = x.mean(-1, keepdims=True)
        d = x - mean
        self.sigma = np.sqrt((d * d).mean(-1, keepdims=True) + eps)
        self.xhat = d / self.sigma
        self.xmax = np.abs(x).max(-1, keepdims=True)
        self.out = self.xhat * self.gamma + self.beta

    def unit(self):
        return U24 * (np.abs(self.gamma) * (self.xmax / self.sigma + np.abs(self.xhat)) + np.abs(self.out))

    def bound(self):
        t = GAMMA["layernorm"] * self.unit()
        return final_rounding(self.out, t) + t


def layernorm_f32(parts, gamma, beta, eps, mutant=None):
    """The kernel's arithmetic in float32 (two-pass statistics), before the final rounding.  Mutants: 'n_minus_1', 'eps1e-5'."""
    x = f32(parts[0])
    for p in parts[1:]:
        x = x + f32(p)
    n = x.shape[-1]
    mean = x.sum(-1, keepdims=True, dtype=np.float32) / np.float32(n)
    d = x - mean
    var = (d * d).sum(-1, keepdims=True, dtype=np.float32) / np.float32(n - 1 if mutant == "n_minus_1" else n)
    rstd = np.float32(1) / np.sqrt(var + np.float32(1e-5 if mutant == "eps1e-5" else eps), dtype=np.float32)
    return d * rstd * f32(gamma) + f32(beta)


def layernorm_case(cols, rows, family):
    """(x, bias, residual, gamma, beta, eps) as fp16 arrays + the eps the kernel is called with."""
    r = rng_of("ln", cols, rows, family)
    z = lambda *s: r.standard_normal(s)
    eps = 1e-5 if family == "tiny_eps1e-5" else 1e-12
    if family == "normal":
        x, bias, res = z(rows, cols), z(cols), z(rows, cols)
    elif family == "mean30":
        x, bias, res = 18 + 0.6 * z(rows, cols), 2 + 0.5 * z(cols), 10 + 0.6 * z(rows, cols)
    elif family.startswith("tiny"):                 # sigma = 2^-9 around 1.0: eps = 1e-5 is no longer negligible
        x, bias, res = 0.5 + 2.0 ** -9.5 * z(rows, cols), 2.0 ** -12 * z(cols), 0.5 + 2.0 ** -9.5 * z(rows, cols)
    elif family == "scale100":
        x, bias, res = 70 * z(rows, cols), 10 * z(cols), 70 * z(rows, cols)
    else:
        raise ValueError(family)
    gamma, beta = 1 + 0.3 * z(cols), 0.5 * z(cols)
    return h16(x), h16(bias), h16(res), h16(gamma), h16(beta), eps


def layernorm_cases():
    for cols in LN_COLS:
        for rows in LN_ROWS:
            for family in LN_FAMILIES:
                yield (cols, rows, family), layernorm_case(cols, rows, family)


def constant_rows_case(cols, rows):
    """x + bias + residual is the same value in every column of a row: every fp32 sum is exact, the deviation is 0 and the
    output equals beta bit for bit."""
    r = rng_of("const", cols, rows)
    x = np.repeat(np.array([3.25, -0.5, 100.0, 0.0, 2.0 ** -10, -7.0, 1.0, 0.125, 33.0])[:rows, None], cols, 1)
    bias = np.full(cols, 0.5)
    res = np.repeat(np.array([-1.125, 2.0, 28.0, 0.0, 0.0, -7.0, 0.0, 0.0, 0.75])[:rows, None], cols, 1)
    gamma, beta = 1 + 0.3 * r.standard_normal(cols), 0.5 * r.standard_normal(cols) + 0.01
    return h16(x), h16(bias), h16(res), h16(gamma), h16(beta)


EMBED_CASES = (   # hidden, batch, seq_len  (n_tokens = batch * seq_len: 15, 35, 6, 21, 9 -- none a multiple of 4)
    (8, 3, 5), (520, 5, 7), (768, 2, 3), (1016, 3, 7), (1024, 1, 9),
)
EMBED_VOCAB, EMBED_TYPES = 37, 3


def embed_case(hidden, batch, seq_len):
    """Tables, ids and type ids (some outside their range: those read row 0), lengths for the packed layout."""
    r = rng_of("embed", hidden, batch, seq_len)
    word = h16(r.standard_normal((EMBED_VOCAB, hidden)))
    pos = h16(0.5 * r.standard_normal((seq_len, hidden)))
    types = h16(0.5 * r.standard_normal((EMBED_TYPES, hidden)))
    gamma, beta = h16(1 + 0.3 * r.standard_normal(hidden)), h16(0.5 * r.standard_normal(hidden))
    ids = r.integers(0, EMBED_VOCAB, (batch, seq_len)).astype(np.int64)
    type_ids = r.integers(0, EMBED_TYPES, (batch, seq_len)).astype(np.int64)
    flat_i, flat_t = ids.reshape(-1), type_ids.reshape(-1)
    flat_i[0], flat_i[-1], flat_i[len(flat_i) // 2] = -1, EMBED_VOCAB, 2 ** 40
    flat_t[1], flat_t[-1], flat_t[len(flat_t) // 2] = -5, EMBED_TYPES, 2 ** 33
    lens = r.integers(1, seq_len + 1, batch).astype(np.int32)
    lens[0] = seq_len
    return dict(word=word, pos=pos, types=types, gamma=gamma, beta=beta, ids=ids, type_ids=type_ids, lens=lens)


def embed_parts(c, typed):
    """The three fp16 rows every token sums, [batch * seq_len, hidden] each, by the header's rules."""
    ids = np.where((c["ids"] < 0) | (c["ids"] >= EMBED_VOCAB), 0, c["ids"]).reshape(-1)
    tt = np.where((c["type_ids"] < 0) | (c["type_ids"] >= EMBED_TYPES), 0, c["type_ids"]).reshape(-1)
    if not typed:
        tt = np.zeros_like(tt)
    batch, seq_len = c["ids"].shape
    position = np.arange(batch * seq_len) % seq_len
    return c["word"][ids], c["pos"][position], c["types"][tt]


def packed_rows(lens, seq_len):
    """Padded token index of every packed row, in order."""
    return np.concatenate([b * seq_len + np.arange(n) for b, n in enumerate(lens)])


# ------------------------------------------------------------------------------------------------------------------
# erf-GELU
# ------------------------------------------------------------------------------------------------------------------
def gelu_ref(t):
    t = torch.from_numpy(f64(t))
    return (0.5 * t * (1.0 + torch.special.erf(t / math.sqrt(2.0)))).numpy()


def gelu_unit(t):
    return U24 * np.abs(t) * (1 + np.abs(t))


def gelu_bound(t, t_err=0.0):
    """t: the float64 argument; t_err: what the argument itself may be off by (0 for bias_gelu: x + bias is exact in fp32).
    |gelu'| <= 1.13."""
    ref = gelu_ref(t)
    e = 1.13 * t_err + GAMMA["gelu"] * gelu_unit(t)
    return final_rounding(ref, e) + e


def gelu_f32(t, mutant=None):
    """float32 restatement on a float32 argument.  Mutant 'tanh': the tanh form."""
    t = torch.from_numpy(f32(t))
    if mutant == "tanh":
        y = 0.5 * t * (1.0 + torch.tanh(np.float32(math.sqrt(2.0 / math.pi)) * (t + np.float32(0.044715) * t * t * t)))
    else:
        y = np.float32(0.5) * t * (np.float32(1.0) + torch.special.erf(t * np.float32(0.70710678118654752440)))
    return y.numpy()


def gelu_mismatches(got, x, bias):
    """Boolean map of the outputs outside the bound.  Where the correctly rounded result is not finite (x + bias beyond
    fp16's range) the output must be that infinity."""
    t = f64(x) + f64(bias)
    ref = gelu_ref(t)
    with np.errstate(over="ignore"):
        expect = f64(h16(ref))
    got = f64(got)
    return np.where(np.isfinite(expect), ~(np.abs(got - ref) <= gelu_bound(t)), got != expect)


def gelu_x_all_finite():
    """All 63 488 finite fp16 bit patterns (both zeros, the subnormals), as [8, 7936]."""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    x = x[np.isfinite(x)]
    assert x.size == 63488
    return x.reshape(8, 7936)


GELU_BIAS_VALUES = (0.0, -0.0, 0.5, -0.5, 2.0 ** -14, -(2.0 ** -24), 1e-3, -3e-2, 2.0, -2.0, 32.0, -32.0, 0.25, -0.125, 7e-3, 1.0)


def gelu_cases():
    x = gelu_x_all_finite()
    yield "bias0", x, np.zeros(x.shape[1], np.float16)
    yield "mixed", x, h16(np.resize(np.array(GELU_BIAS_VALUES), x.shape[1]))


# ------------------------------------------------------------------------------------------------------------------
# Masked multi-head attention with the folded Q|K|V bias (proqa_attention_ex_f16's contract)
# ------------------------------------------------------------------------------------------------------------------
HEAD = 64
EDGE_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 255, 256, 257)


def clamp_lens(lens, S):
    return np.clip(np.asarray(lens, dtype=np.int64), 1, S)


class AttentionRef:
    """Float64 attention over the valid keys.  qkv fp16 [B, S, 3 * NH * 64] in the padded layout (rows >= len are never
    read here), bias fp16 [3 * NH * 64] or None.  q + b_q is rounded once to fp16, the key bias is absent, the value bias is
    added to the output.  cls_only: query 0 only.  out [B, Sq, NH * 64]; only queries < len are meaningful.

    bound() is the full kernel's (attention_fwd).  The [CLS] kernel (attention_cls_fwd) rounds elsewhere, and bound_cls()
    says where: it keeps the probabilities in fp32 and rounds the output once, but with a bias it reads k + b_k and
    v + b_v, each rounded to fp16 -- what a half-precision dense layer would have stored.  The value rounding moves an
    output by at most sum_j P_j ulp16(v_j + b_v) / 2.  The key rounding moves the score of key j by at most
    delta_j = sum_d |q_d| ulp16(k_jd + b_kd) / 2 / 8, every probability by a factor within exp(+-2 max_j delta_j), and the
    output by at most (exp(2 max_j delta_j) - 1) sum_j P_j |v_j - out| (the changes of the probabilities sum to 0).  A key
    bias is mathematically absent, but one of 40 costs every key the bits below 2^-5 and this bound says so."""

    def __init__(self, qkv, bias, lens, NH, cls_only=False):
        B, S = qkv.shape[:2]
        H = NH * HEAD
        x = np.asarray(qkv).reshape(B, S, 3, NH, HEAD)
        lens = clamp_lens(lens, S)
        Sq = 1 if cls_only else S
        self.ctx = np.zeros((B, Sq, NH, HEAD))
        self.pv = np.zeros((B, Sq, NH, HEAD))        # sum_j P_j |v_j|
        self.sub = np.zeros((B, Sq, NH, HEAD))       # rounding of the probabilities to fp16
        self.smax = np.zeros((B, Sq, NH, 1))
        self.cls_rounding = np.zeros((B, 1, NH, HEAD))   # query 0: the fp16 roundings of k + b_k and v + b_v
        for b in range(B):
            n = int(lens[b])
            for h in range(NH):
                q = x[b, :Sq, 0, h]
                if bias is not None:
                    q = (q.astype(np.float32) + np.asarray(bias)[h * HEAD:(h + 1) * HEAD].astype(np.float32)).astype(np.float16)
                q, k, v = f64(q), f64(x[b, :n, 1, h]), f64(x[b, :n, 2, h])
                s = q @ k.T / 8.0
                p = np.exp(s - s.max(-1, keepdims=True))
                l = p.sum(-1, keepdims=True)
                self.ctx[b, :, h] = (p / l) @ v
                self.pv[b, :, h] = (p / l) @ np.abs(v)
                self.sub[b, :, h] = (np.maximum(2.0 ** -11 * p, 2.0 ** -25) / l) @ np.abs(v)
                self.smax[b, :, h] = np.abs(s).max(-1, keepdims=True)
                if bias is not None:
                    bk, bv = (f64(np.asarray(bias)[i * H + h * HEAD:i * H + (h + 1) * HEAD]) for i in (1, 2))
                    P0 = (p / l)[:1]
                    delta = (np.abs(q[:1]) @ (ulp16(k + bk) / 2).T / 8.0).max()
                    self.cls_rounding[b, 0, h] = (P0 @ (ulp16(v + bv) / 2) + np.expm1(2 * delta) * (P0 @ np.abs(v - P0 @ v)))[0]
        self.bias_v = None if bias is None else f64(np.asarray(bias)[2 * H:]).reshape(NH, HEAD)
        self.shape = (B, Sq, H)
        self.lens = lens

    @property
    def out(self):
        return (self.ctx if self.bias_v is None else self.ctx + self.bias_v).reshape(self.shape)

    def unit(self):
        return (U24 * self.pv * (1 + self.smax)).reshape(self.shape)

    def bound(self):
        t = self.sub + GAMMA["attention"] * U24 * self.pv * (1 + self.smax)
        if self.bias_v is None:
            return (final_rounding(self.ctx, t) + t).reshape(self.shape)
        t = t + final_rounding(self.ctx, t)          # the context is rounded to fp16, then the bias is added in fp16
        return (final_rounding(self.ctx + self.bias_v, t) + t).reshape(self.shape)

    def bound_cls(self):
        """[B, 1, H]: the [CLS] kernel's bound for query 0."""
        t = self.cls_rounding + GAMMA["attention"] * U24 * (self.pv * (1 + self.smax))[:, :1]
        ref = self.ctx[:, :1] if self.bias_v is None else self.ctx[:, :1] + self.bias_v
        return (final_rounding(ref, t) + t).reshape(self.shape[0], 1, self.shape[2])

    def valid(self):
        """[B, Sq] mask of the queries that exist."""
        return np.arange(self.shape[1])[None, :] < self.lens[:, None]


def attention_f32(qkv, bias, lens, NH, mutant=None, round_p=True, final=True):
    """The full kernel's arithmetic in float32: 32-key tiles in order, running maximum and sum, exp2 of the unscaled score,
    probabilities rounded to fp16 for P V (round_p), rescale whenever the maximum moves.  final: round the context to fp16 and
    add the value bias in fp16, as the kernel stores it; else the fp32 context (+ bias) before any output rounding.
    Mutants: 'mask_le' (key <= len is valid), 'drop_last' (the last valid key is masked), 'no_rescale_at_chunk' (the
    accumulators are not rescaled when the maximum moves in the first tile of a 128-key chunk)."""
    B, S = qkv.shape[:2]
    H = NH * HEAD
    x = np.asarray(qkv).reshape(B, S, 3, NH, HEAD)
    lens = clamp_lens(lens, S)
    c = np.float32(0.125 * 1.4426950408889634)
    out = np.zeros((B, S, NH, HEAD), np.float32)
    for b in range(B):
        n = int(lens[b])
        n_keys = min(n + 1, S) if mutant == "mask_le" else (max(n - 1, 1) if mutant == "drop_last" else n)
        for h in range(NH):
            q = x[b, :, 0, h]
            if bias is not None:
                q = (f32(q) + f32(np.asarray(bias)[h * HEAD:(h + 1) * HEAD])).astype(np.float16)
            q, k, v = f32(q), f32(x[b, :, 1, h]), f32(x[b, :, 2, h])
            m = np.full((S, 1), -np.inf, np.float32)
            l = np.zeros((S, 1), np.float32)
            o = np.zeros((S, HEAD), np.float32)
            for t0 in range(0, n_keys, 32):
                t1 = min(t0 + 32, n_keys)
                s = q @ k[t0:t1].T
                m_new = np.maximum(m, s.max(-1, keepdims=True))
                p = np.exp2(s * c - m_new * c, dtype=np.float32)
                with np.errstate(invalid="ignore"):
                    alpha = np.where(np.isinf(m), np.float32(0), np.exp2((m - m_new) * c, dtype=np.float32))
                if mutant == "no_rescale_at_chunk" and t0 and t0 % 128 == 0:
                    alpha = np.ones_like(alpha)
                l = l * alpha + p.sum(-1, keepdims=True, dtype=np.float32)
                o = o * alpha + (f32(p.astype(np.float16)) if round_p else p) @ v[t0:t1]
                m = m_new
            out[b, :, h] = o / l
    if bias is None:
        return h16(out).reshape(B, S, H) if final else out.reshape(B, S, H)
    bv = np.asarray(bias)[2 * H:].reshape(NH, HEAD)
    if final:
        return (f32(h16(out)) + f32(bv)).astype(np.float16).reshape(B, S, H)
    return (out + f32(bv)).reshape(B, S, H)


def attention_cls_f32(qkv, bias, lens, NH, mutant=None):
    """The [CLS] kernel's arithmetic in float32, query 0 only: q + b_q, k + b_k and v + b_v rounded to fp16, fp32 scores,
    softmax and P V, one rounding of the output.  Mutant 'skip_group_tail': the keys of a last, partial 8-key group are lost."""
    B, S = qkv.shape[:2]
    H = NH * HEAD
    x = np.asarray(qkv).reshape(B, S, 3, NH, HEAD)
    lens = clamp_lens(lens, S)
    out = np.zeros((B, 1, NH, HEAD), np.float16)
    for b in range(B):
        n = int(lens[b])
        for h in range(NH):
            q, k, v = x[b, 0, 0, h], x[b, :n, 1, h], x[b, :n, 2, h]
            if bias is not None:
                bq, bk, bv = (np.asarray(bias)[i * H + h * HEAD:i * H + (h + 1) * HEAD] for i in range(3))
                q, k, v = ((f32(a) + f32(c)).astype(np.float16) for a, c in ((q, bq), (k, bk), (v, bv)))
            if mutant == "skip_group_tail" and n >= 8:
                k, v = k[:n - n % 8], v[:n - n % 8]
            s = (f32(k) * f32(q)).sum(-1, dtype=np.float32) * np.float32(0.125)
            p = np.exp(s - s.max(), dtype=np.float32)
            out[b, 0, h] = ((p[:, None] * f32(v)).sum(0, dtype=np.float32) / p.sum(dtype=np.float32)).astype(np.float16)
    return out.reshape(B, 1, H)


PLANT = np.where(np.arange(HEAD) % 3 == 0, -1.0, 1.0)        # the direction of the planted keys


def attention_inputs(name, B, S, NH, lens, scale=1.0, with_bias=False, plant=True, zero_q=False, key_bias=None):
    """qkv [B, S, 3H] fp16 in the padded layout, bias or None.  plant: in every (sequence, head) the LAST VALID key carries the
    dominant score (16 above the others' N(0, 1)) for every third query (from query 0 in the even sequences, from query 1 in
    the odd ones: the [CLS] kernel sees planted and ordinary softmax rows), with V = 50 + d / 4; the FIRST MASKED key (row len,
    where it exists: padded layout only) carries twice that score and V = -60000 -- a kernel that reads one key too many or
    too few moves those queries by tens."""
    r = rng_of("attn", name)
    H = NH * HEAD
    x = r.standard_normal((B, S, 3, NH, HEAD))
    x[:, :, 0] *= scale
    if zero_q:
        x[:, :, 0] = 0.0
    lens_c = clamp_lens(lens, S)
    if plant:
        for b in range(B):
            n = int(lens_c[b])
            x[b, b % 2::3, 0] += PLANT * scale      # (query 0 -- all the [CLS] kernel evaluates -- in every other sequence)
            x[b, n - 1, 1] = 2.0 * PLANT
            x[b, n - 1, 2] = 50.0 + np.arange(HEAD) / 4.0
            if n < S:
                x[b, n, 1] = 4.0 * PLANT
                x[b, n, 2] = -60000.0
    bias = None
    if with_bias:
        bias = 0.5 * r.standard_normal(3 * H)
        if zero_q:
            bias[:H] = 0.0
        if key_bias is not None:
            bias[H:2 * H] = key_bias
        bias = h16(bias)
    return h16(x.reshape(B, S, 3 * H)), bias


def _attn(name, B, S, NH, lens, **kw):
    return dict(name=name, B=B, S=S, NH=NH, lens=np.asarray(lens, dtype=np.int32), kw=kw)


def attention_cases():
    """The case list of the GPU tests (both layouts and both kernels run every one that applies) and of the measurement."""
    cases = []
    for NH in (1, 2):
        for with_bias in (False, True):
            cases.append(_attn(f"edges_nh{NH}_bias{int(with_bias)}", 16, 257, NH, EDGE_LENS, with_bias=with_bias))
    for pairs in (1, 7, 8, 9, 17):                    # blockIdx -> (XCD, pair, query chunk); 4 pairs per [CLS] workgroup
        for S in (64, 200, 300):                      # 1, 2, 3 query chunks
            r = rng_of("lens", pairs, S)
            lens = r.integers(1, S + 1, pairs)
            lens[0] = S
            cases.append(_attn(f"pairs{pairs}_S{S}", pairs, S, 1, lens, with_bias=(pairs % 2 == 1)))
    cases.append(_attn("cls_groups", 3, 9, 1, (7, 8, 9)))
    cases.append(_attn("cls_groups_nh3", 3, 12, 3, (7, 8, 9), with_bias=True))
    short = (1, 33, 128, 129, 257)
    cases.append(_attn("scale3", 5, 257, 1, short, scale=3.0))
    cases.append(_attn("scale8", 5, 257, 1, short, scale=8.0, with_bias=True))
    cases.append(_attn("zero_q", 5, 257, 1, short, zero_q=True, plant=False))
    cases.append(_attn("zero_q_bias", 5, 257, 2, short, zero_q=True, plant=False, with_bias=True))
    cases.append(_attn("key_bias40", 5, 257, 2, short, with_bias=True, key_bias=40.0))
    return cases


def attention_case_inputs(case):
    return attention_inputs(case["name"], case["B"], case["S"], case["NH"], case["lens"], **case["kw"])


# ------------------------------------------------------------------------------------------------------------------
# Dense layer (small_dense_mfma: y = act(x w^T + bias)) and pooler + projection (cls_dense_mfma twice)
# ------------------------------------------------------------------------------------------------------------------
DENSE_M = (1, 31, 32, 33, 255, 256, 257)
DENSE_N = (32, 96, 768)
DENSE_K = (128, 256, 768, 3072)


def dense_inputs(M, N, K, kind):
    """kind 'int': small integers, every fp32 partial sum exact (|sum| <= 3072 * 9 < 2^24) and the result an fp16 integer
    only when small -- so the weights are sparse enough to keep |y| <= 2048; 'gauss': N(0, 1) x N(0, 1/K)."""
    r = rng_of("dense", M, N, K, kind)
    if kind == "int":
        x = r.integers(-3, 4, (M, K)).astype(np.float64)
        w = r.integers(-3, 4, (N, K)) * (r.random((N, K)) < 64.0 / K)
        bias = r.integers(-4, 5, N).astype(np.float64)
    else:
        x = r.standard_normal((M, K))
        w = r.standard_normal((N, K)) / math.sqrt(K)
        bias = 0.5 * r.standard_normal(N)
    return h16(x), h16(w), h16(bias)


class DenseRef:
    def __init__(self, x, w, bias=None, act=0):
        self.pre = f64(x) @ f64(w).T
        self.mag = np.abs(f64(x)) @ np.abs(f64(w)).T
        if bias is not None:
            self.pre = self.pre + f64(bias)
            self.mag = self.mag + np.abs(f64(bias))
        self.act = act
        self.out = gelu_ref(self.pre) if act == 1 else self.pre

    def unit(self):
        return U24 * self.mag

    def bound(self, out32=False):
        t = GAMMA["dense"] * self.unit()
        if self.act == 1:
            return gelu_bound(self.pre, t_err=t)
        return final_rounding(self.out, t, out32) + t


def dense_f32(x, w, bias=None, act=0, mutant=None):
    """float32 restatement before the output rounding.  Mutant 'skip_last_32k'."""
    K = x.shape[1] - (32 if mutant == "skip_last_32k" else 0)
    y = f32(x)[:, :K] @ f32(w)[:, :K].T
    if bias is not None:
        y = y + f32(bias)
    return gelu_f32(y) if act == 1 else y


def dense_cases():
    for M in DENSE_M:
        for N in DENSE_N:
            for K in DENSE_K:
                yield M, N, K


POOL_HIDDEN = (32, 96, 128, 160, 768)
POOL_BATCH = (1, 31, 32, 33, 65)
EMBED_DIM = 128


def pooler_inputs(hidden, batch, seq_len=3, saturate=False):
    """h [B, S, hidden] (only row 0 of a sequence is read), pooler and projection weights.  saturate: pre-activations up to
    |20|, where tanh is 1 to fp32 precision."""
    r = rng_of("pool", hidden, batch, saturate)
    h = r.standard_normal((batch, seq_len, hidden))
    wp = r.standard_normal((hidden, hidden)) / math.sqrt(hidden) * (6.0 if saturate else 1.0)
    bp = 0.3 * r.standard_normal(hidden)
    wj = r.standard_normal((EMBED_DIM, hidden)) / math.sqrt(hidden)
    bj = 0.3 * r.standard_normal(EMBED_DIM)
    return tuple(h16(a) for a in (h, wp, bp, wj, bj))


def pooler_integer_inputs(hidden, batch, seq_len=3):
    """Pre-activations in {-32, 0, 32}: tanh is -1, 0, 1 exactly in fp32, and the projection of integers is exact."""
    r = rng_of("poolint", hidden, batch)
    h = r.integers(-2, 3, (batch, seq_len, hidden)).astype(np.float64)
    h[:, 0, 0] = r.choice([-1.0, 1.0], batch)
    wp = np.zeros((hidden, hidden))
    wp[:, 0] = 32.0 * r.integers(-1, 2, hidden)
    bp = np.zeros(hidden)
    wj = r.integers(-3, 4, (EMBED_DIM, hidden)).astype(np.float64)
    bj = r.integers(-4, 5, EMBED_DIM).astype(np.float64)
    expect = (h[:, 0, :1] * np.sign(wp[:, 0])[None, :]) @ wj.T + bj
    return tuple(h16(a) for a in (h, wp, bp, wj, bj)), expect


class PoolerRef:
    def __init__(self, h, wp, bp, wj, bj):
        x = f64(h)[:, 0]
        self.pre = x @ f64(wp).T + f64(bp)
        self.pre_mag = np.abs(x) @ np.abs(f64(wp)).T + np.abs(f64(bp))
        self.pooled = np.tanh(self.pre)
        self.wj = f64(wj)
        self.out = self.pooled @ self.wj.T + f64(bj)
        self.out_mag = np.abs(self.pooled) @ np.abs(self.wj).T + np.abs(f64(bj))

    def pooled_err(self):
        """What the stored fp16 pooled value may be off by: the fp32 sum through tanh' <= 1, tanhf itself (|tanh| <= 1), and
        the rounding to fp16."""
        t = GAMMA["pooler"] * U24 * (self.pre_mag + 1.0)
        return t + final_rounding(self.pooled, t)

    def unit(self):
        return U24 * ((self.pre_mag + 1.0) @ np.abs(self.wj).T + self.out_mag)

    def bound(self, out32):
        t = self.pooled_err() @ np.abs(self.wj).T + GAMMA["pooler"] * U24 * self.out_mag
        return final_rounding(self.out, t, out32) + t


def pooler_f32(h, wp, bp, wj, bj, round_pooled=True):
    """float32 restatement: the pooled row is stored as fp16 between the two products (round_pooled)."""
    pooled = np.tanh(f32(h)[:, 0] @ f32(wp).T + f32(bp), dtype=np.float32)
    if round_pooled:
        pooled = f32(pooled.astype(np.float16))
    return pooled @ f32(wj).T + f32(bj)


def pooler_cases():
    for hidden in POOL_HIDDEN:
        for batch in POOL_BATCH:
            for saturate in (False, True):
                yield hidden, batch, saturate


# ------------------------------------------------------------------------------------------------------------------
# The measurement behind GAMMA
# ------------------------------------------------------------------------------------------------------------------
def _ratio(diff, unit):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(unit > 0, np.abs(diff) / unit, np.where(diff == 0, 0.0, np.inf))
    return float(r.max())


def measure_reference_error(verbose=False):
    """Worst |float32 restatement - float64| / unit per operator, over the case lists of the GPU tests.  The restatements run
    WITHOUT the documented intermediate roundings (those have their own term in the bound), before the output rounding."""
    worst = {op: 0.0 for op in REFERENCE_RATIO}

    def note(op, case, r):
        worst[op] = max(worst[op], r)
        if verbose:
            print(f"  {op:10s} {str(case):40s} {r:8.3f}")

    for key, (x, bias, res, gamma, beta, eps) in layernorm_cases():
        ref = LayerNormRef((x, bias, res), gamma, beta, eps)
        note("layernorm", key, _ratio(layernorm_f32((x, bias, res), gamma, beta, eps) - ref.out, ref.unit()))
    for hidden, batch, seq_len in EMBED_CASES:
        c = embed_case(hidden, batch, seq_len)
        parts = embed_parts(c, typed=True)
        ref = LayerNormRef(parts, c["gamma"], c["beta"], 1e-12)
        note("layernorm", ("embed", hidden), _ratio(layernorm_f32(parts, c["gamma"], c["beta"], 1e-12) - ref.out, ref.unit()))
    for name, x, bias in gelu_cases():
        t = f64(x) + f64(bias)
        got = f64(gelu_f32(f32(x) + f32(bias)))
        note("gelu", name, _ratio(got - gelu_ref(t), gelu_unit(t)))
    for case in attention_cases():
        qkv, bias = attention_case_inputs(case)
        ref = AttentionRef(qkv, bias, case["lens"], case["NH"])
        got = attention_f32(qkv, bias, case["lens"], case["NH"], round_p=False, final=False)
        v = ref.valid()
        note("attention", case["name"], _ratio((got - ref.out)[v], ref.unit()[v]))
    for M, N, K in dense_cases():
        x, w, bias = dense_inputs(M, N, K, "gauss")
        ref = DenseRef(x, w, bias)
        note("dense", (M, N, K), _ratio(dense_f32(x, w, bias) - ref.out, ref.unit()))
    for hidden, batch, saturate in pooler_cases():
        args = pooler_inputs(hidden, batch, saturate=saturate)
        ref = PoolerRef(*args)
        note("pooler", (hidden, batch, saturate), _ratio(pooler_f32(*args, round_pooled=False) - ref.out, ref.unit()))
    return worst


if __name__ == "__main__":
    w = measure_reference_error(verbose=True)
    for op, r in w.items():
        print(f'    "{op}": {r:.4f},      # GAMMA = {4 * r:.4f}')
