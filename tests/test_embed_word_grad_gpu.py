"""The deterministic word-embedding gradient (proqa_embed_layernorm_[typed_]varlen_backward_det_f16, csrc/train_kernels.hip):
d_word summed in a fixed order instead of with fp32 atomics.

The contract (include/proqa_hip.h): the occurrences of a word id, in ascending packed row, are cut into chunks of
C = proqa_embed_word_grad_chunk(); a chunk's partial is the sequential fp32 sum of its tokens' dz, the id's sum the sequential
fp32 sum of the partials, and that sum is added once into d_word[id].  Every other output carries the bits of the atomic entry
point.

Oracles: tests/train_oracle.py (untyped) and tests/reader_train_oracle.py (typed), float64 on the kernels' fp16 inputs; error
measure max|gpu - ref| / max|ref| per output tensor, as in the tests of the atomic entry points.

Tolerance of d_word: the bounds of those tests, unchanged -- untyped BOUNDS["embed"]["d_word"] of test_train_ops_gpu.py
(4 x 1.449e-07), typed 4 x REFERENCE_ERROR["d_word"] of test_embed_typed_backward_gpu.py (4 x 2.124e-07): four times the
measured error of the reference's own arithmetic (fp32 sums on fp16 inputs).  A fixed-order fp32 sum is no worse than an
atomic one.  The other outputs are compared bit for bit with the atomic entry point, which the existing tests hold to the
oracle.

Shapes: the EMBED_CASES of test_train_ops_gpu.py (T = 300, vocabulary 50: every id dozens of times, several chunks per id);
a ragged batch of 24 sequences (lengths cycling 512, 1, 300, 511, 64, 257: T = 6580 = 3 x 2048 + 436, a sort workgroup takes
2048 keys) at hidden 128 with vocabulary 50 (one radix pass, ~130 occurrences per id) and 30522 (two passes, mostly single
occurrences next to a few frequent ids); 4 x 512 tokens of ONE id (128 chunks, the longest chain of partials); one token.
"""
import functools

import numpy as np
import pytest
import torch

import reader_train_oracle as typed_oracle
import train_oracle as oracle
from test_embed_typed_backward_gpu import REFERENCE_ERROR as TYPED_REFERENCE_ERROR
from test_train_ops_gpu import BOUNDS as UNTYPED_BOUNDS
from test_train_ops_gpu import EMBED_CASES, EMBED_USED, EMBED_VOCAB, embed_case

pytestmark = pytest.mark.gpu

D_WORD_BOUND = {False: UNTYPED_BOUNDS["embed"]["d_word"], True: 4.0 * TYPED_REFERENCE_ERROR["d_word"]}
OUTPUTS = ("dgamma", "dbeta", "d_word", "d_pos", "d_types")       # untyped: d_types is the type-0 row [hidden]
OTHERS = ("dgamma", "dbeta", "d_pos", "d_types")
SORT_WORKGROUP_KEYS = 2048
RAGGED_LENS = (512, 1, 300, 511, 64, 257) * 4
EINVAL = -1


def rng_f16(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).half()


def bits(t):
    return t.view(torch.int32)


def cu_of(lens, dev):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)


def segments(lens, seq_len):
    """type ids of [CLS] q [SEP] p [SEP]: the first third of every sequence is type 0, the rest type 1"""
    question = torch.tensor([max(1, n // 3) for n in lens])[:, None]
    return (torch.arange(seq_len)[None] >= question).long().expand(len(lens), seq_len).contiguous()


def make_case(seed, hidden, lens, vocab, ids=None, positions=None):
    """CPU tensors of one case (no reference): a two-row type table, segment type ids"""
    g = torch.Generator().manual_seed(seed)
    S = max(lens)
    if ids is None:
        ids = torch.randint(0, vocab, (len(lens), S), generator=g)
    return dict(dy=rng_f16(seed + 1, sum(lens), hidden), ids=ids, type_ids=segments(lens, S), lens=tuple(lens),
                word=rng_f16(seed + 2, vocab, hidden), pos=rng_f16(seed + 3, positions or S, hidden),
                types=rng_f16(seed + 4, 2, hidden), gamma=(1.0 + 0.1 * torch.randn(hidden, generator=g)).half(), eps=1e-12)


def reference(c, typed):
    if typed:
        return typed_oracle.embed_typed_backward(**c)
    ref = oracle.embed_layernorm_backward(c["dy"], c["ids"], c["lens"], c["word"], c["pos"], c["types"][0], c["gamma"], c["eps"])
    ref["d_types"] = ref.pop("d_type0")
    return ref


@functools.lru_cache(maxsize=None)
def embed_cases_case(hidden, lens, typed):
    """the case of test_train_ops_gpu.py (its type-0 row is row 0 of the table here) and its reference"""
    c, ref = embed_case(hidden, lens)
    c = {k: v for k, v in c.items() if k != "type0"}
    c.update(types=torch.stack([embed_case(hidden, lens)[0]["type0"], rng_f16(hidden + 5, hidden)]),
             type_ids=segments(lens, max(lens)))
    if typed:
        return c, reference(c, True)
    ref = dict(ref)
    ref["d_types"] = ref.pop("d_type0")
    return c, ref


@functools.lru_cache(maxsize=None)
def ragged_case(vocab, typed):
    """24 ragged sequences, hidden 128; ids skewed to the small ones, a [CLS]-like id at position 0 and a [SEP]-like one at
    the end of every sequence"""
    lens = RAGGED_LENS
    T = sum(lens)
    assert T > SORT_WORKGROUP_KEYS and T % SORT_WORKGROUP_KEYS != 0
    g = torch.Generator().manual_seed(vocab)
    ids = (vocab * torch.rand((len(lens), max(lens)), generator=g, dtype=torch.float64) ** 3).long().clamp_(max=vocab - 1)
    ids[:, 0] = 11
    for b, n in enumerate(lens):
        ids[b, n - 1] = 12
    c = make_case(vocab + 1, 128, lens, vocab, ids=ids)
    return c, reference(c, typed)


def run(dev, c, typed, deterministic=True):
    from proqa_amd import trainable as T
    d = {k: v.to(dev) for k, v in c.items() if torch.is_tensor(v)}
    if typed:
        out = T.embed_layernorm_typed_backward(d["dy"], d["ids"], d["type_ids"] if c.get("type_ids") is not None else None,
                                               cu_of(c["lens"], dev), d["word"], d["pos"], d["types"], d["gamma"], c["eps"],
                                               deterministic=deterministic)
    else:
        out = T.embed_layernorm_backward(d["dy"], d["ids"], cu_of(c["lens"], dev), d["word"], d["pos"],
                                         d["types"][0].contiguous(), d["gamma"], c["eps"], deterministic=deterministic)
    return dict(zip(OUTPUTS, out))


def new_outputs(dev, c, typed, fill):
    H = c["word"].shape[1]
    return {"dgamma": torch.full((H,), fill, device=dev), "dbeta": torch.full((H,), fill, device=dev),
            "d_word": torch.full(c["word"].shape, fill, device=dev), "d_pos": torch.full(c["pos"].shape, fill, device=dev),
            "d_types": torch.full(c["types"].shape if typed else (H,), fill, device=dev)}


def raw_call(dev, c, typed, *, out=None, fill=0.0, n_types=None, hidden=None, seq_len=None, ws_bytes=None, null=None):
    """The *_det entry point itself over `out` (or buffers filled with `fill`) -> (status, outputs).  null: the name of an
    argument passed as NULL."""
    from proqa_amd import _lib
    lib = _lib.load()
    d = {k: v.to(dev) for k, v in c.items() if torch.is_tensor(v)}
    batch, S = c["ids"].shape
    H = c["word"].shape[1]
    T = sum(c["lens"])
    out = new_outputs(dev, c, typed, fill) if out is None else out
    need = lib.proqa_embed_layernorm_backward_det_workspace_bytes(T, H, int(typed))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    p = {"dy": d["dy"].data_ptr(), "ids": d["ids"].data_ptr(), "cu": cu_of(c["lens"], dev).data_ptr(), "word": d["word"].data_ptr(),
         "pos": d["pos"].data_ptr(), "gamma": d["gamma"].data_ptr(), "ws": ws.data_ptr(),
         "type_ids": d["type_ids"].data_ptr() if c.get("type_ids") is not None else None,
         "types": d["types"].data_ptr(), **{k: v.data_ptr() for k, v in out.items()}}
    if null is not None:
        p[null] = None
    sizes = (batch, S if seq_len is None else seq_len, H if hidden is None else hidden, T)
    tail = (c["eps"], p["dgamma"], p["dbeta"], p["d_word"], p["d_pos"], p["d_types"], p["ws"],
            need if ws_bytes is None else ws_bytes, _lib.current_stream_ptr())
    with torch.cuda.device(dev):
        if typed:
            status = lib.proqa_embed_layernorm_typed_varlen_backward_det_f16(
                p["dy"], p["ids"], p["type_ids"], p["cu"], *sizes, p["word"], c["word"].shape[0], p["pos"], p["types"],
                c["types"].shape[0] if n_types is None else n_types, p["gamma"], *tail)
        else:
            status = lib.proqa_embed_layernorm_varlen_backward_det_f16(
                p["dy"], p["ids"], p["cu"], *sizes, p["word"], c["word"].shape[0], p["pos"], p["types"], p["gamma"], *tail)
    torch.cuda.synchronize(dev)
    return status, out


def check_d_word(got, ref, typed, label):
    err = oracle.rel_err(got.cpu(), ref)
    print(f"{label} d_word: error {err:.3e} bound {D_WORD_BOUND[typed]:.3e}")
    assert err <= D_WORD_BOUND[typed], (label, err, D_WORD_BOUND[typed])


def check_against_both(dev, c, ref, typed, label):
    got = run(dev, c, typed)
    check_d_word(got["d_word"], ref["d_word"], typed, label)
    atomic = run(dev, c, typed, deterministic=False)
    for k in OTHERS:
        assert torch.equal(bits(got[k]), bits(atomic[k])), (label, k)
    again = run(dev, c, typed)
    assert torch.equal(bits(got["d_word"]), bits(again["d_word"])), label
    return got


# ---- 1a: the oracle, and the atomic entry points ---------------------------------------------------------------------------------

@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("hidden,lens", EMBED_CASES)
def test_embed_cases_match_the_oracle_and_the_atomic_entry_point(gpu_device, hidden, lens, typed):
    c, ref = embed_cases_case(hidden, lens, typed)
    got = check_against_both(gpu_device, c, ref, typed, f"embed {hidden} typed={typed}")
    # ids 45 .. 49 appear only past the lengths: their rows are never written
    assert (got["d_word"][EMBED_USED:] == 0).all() and (got["d_word"][:EMBED_USED] != 0).any()
    assert got["d_word"].shape == (EMBED_VOCAB, hidden)


@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("vocab", [50, 30522])
def test_ragged_batch_beyond_one_sort_workgroup(gpu_device, vocab, typed):
    c, ref = ragged_case(vocab, typed)
    got = check_against_both(gpu_device, c, ref, typed, f"ragged vocab={vocab} typed={typed}")
    used = torch.zeros(vocab, dtype=torch.bool)
    for b, n in enumerate(c["lens"]):
        used[c["ids"][b, :n]] = True
    assert (got["d_word"].cpu()[~used] == 0).all()


# ---- 1b: every id once -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("typed", [False, True])
def test_one_occurrence_per_id_is_the_atomic_result_bit_for_bit(gpu_device, typed):
    lens = (40, 7, 1)
    perm = torch.randperm(EMBED_VOCAB, generator=torch.Generator().manual_seed(9))
    ids = torch.full((3, 40), 49)
    at = 0
    for b, n in enumerate(lens):
        ids[b, :n] = perm[at:at + n]
        at += n
    ids[1, 7:] = perm[0]                      # past the length: not an occurrence
    c = make_case(5, 128, lens, EMBED_VOCAB, ids=ids)
    got, atomic = run(gpu_device, c, typed), run(gpu_device, c, typed, deterministic=False)
    for k in OUTPUTS:
        assert torch.equal(bits(got[k]), bits(atomic[k])), k
    check_d_word(got["d_word"], reference(c, typed)["d_word"], typed, "once")


# ---- 1c: the association, bit for bit ----------------------------------------------------------------------------------------------

def contract_sum(rows, C):
    """the contract's sum of the fp32 rows [n, hidden], operation by operation"""
    partials = []
    for first in range(0, len(rows), C):
        acc = rows[first].copy()
        for r in rows[first + 1:first + C]:
            acc = (acc + r).astype(np.float32)
        partials.append(acc)
    total = partials[0]
    for p in partials[1:]:
        total = (total + p).astype(np.float32)
    return total


@functools.lru_cache(maxsize=None)
def association_case(lens, vocab, C):
    """-> (case X: a distinct id per token, case Y: the same tokens with ids mapped many-to-one, word[g(i)] == word[i])"""
    T = sum(lens)
    assert vocab >= T
    rng = np.random.default_rng(T)
    counts = [50 * C + 3, 2 * C + 1, C + 1, C, C - 1, 1]
    left = T - sum(counts)
    assert left > 0
    while left > 0:                               # the rest: small groups
        n = min(left, int(rng.integers(1, 4)))
        counts.append(n)
        left -= n
    pools = [list(rng.permutation(np.arange(r, vocab, 7))) for r in range(7)]       # the ids of each base row
    tokens = rng.permutation(T)
    x, y, at = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64), 0
    for j, n in enumerate(counts):
        members = tokens[at:at + n]
        at += n
        own = [pools[j % 7].pop() for _ in range(n)]
        x[members] = own
        y[members] = own[0]
    assert len(set(x.tolist())) == T
    c = make_case(T, 128, lens, vocab)
    base = rng_f16(T + 9, 7, 128)
    c["word"] = base[torch.arange(vocab) % 7].contiguous()
    S = max(lens)

    def padded(flat):
        ids, row = torch.zeros((len(lens), S), dtype=torch.int64), 0
        for b, n in enumerate(lens):
            ids[b, :n] = torch.from_numpy(flat[row:row + n])
            row += n
        return ids
    return dict(c, ids=padded(x)), dict(c, ids=padded(y)), x, y


@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("lens,vocab", [((512, 1, 300, 200), 8192), (RAGGED_LENS, 30522)])
def test_the_sum_has_the_association_of_the_contract(gpu_device, lens, vocab, typed):
    from proqa_amd import _lib
    C = _lib.load().proqa_embed_word_grad_chunk()
    cx, cy, x, y = association_case(lens, vocab, C)
    counts = np.bincount(y, minlength=vocab)
    assert {1, C - 1, C, C + 1, 2 * C + 1} <= set(counts.tolist()) and counts.max() > 50 * C
    # X through the atomic entry point: one add into a zeroed row leaves dz_t itself in row x[t]
    dz = run(gpu_device, cx, typed, deterministic=False)["d_word"].cpu().numpy()[x]
    want = np.zeros((vocab, 128), dtype=np.float32)
    for k in np.flatnonzero(counts):
        want[k] = np.float32(0.0) + contract_sum(dz[np.flatnonzero(y == k)], C)      # ascending packed row
    got = run(gpu_device, cy, typed)["d_word"].cpu().numpy()
    differ = np.flatnonzero((got.view(np.int32) != want.view(np.int32)).any(axis=1))
    assert differ.size == 0, (differ[:10], counts[differ[:10]])


# ---- 1d: contention and repetition ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def contention_case(hidden, pattern, typed):
    lens = (512, 512, 512, 512)
    c = make_case(hidden + 31, hidden, lens, EMBED_VOCAB)
    if pattern == "one_id":
        c["ids"] = torch.full((4, 512), 7)
    else:                                          # [CLS]-like: position 0 shares an id that occurs nowhere else
        c["ids"] = torch.randint(1, EMBED_USED, (4, 512), generator=torch.Generator().manual_seed(3))
        c["ids"][:, 0] = 0
    return c, reference(c, typed)


@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("pattern", ["one_id", "cls"])
@pytest.mark.parametrize("hidden", [128, 768])
def test_contention_three_runs_into_filled_buffers(gpu_device, hidden, pattern, typed):
    c, ref = contention_case(hidden, pattern, typed)
    runs = []
    for _ in range(3):
        status, out = raw_call(gpu_device, c, typed, fill=3.0)
        assert status == 0
        runs.append(out)
    for other in runs[1:]:
        for k in OUTPUTS:
            assert torch.equal(bits(runs[0][k]), bits(other[k])), k
    check_d_word(runs[0]["d_word"], ref["d_word"] + 3.0, typed, f"{pattern} {hidden} typed={typed} filled")
    unused = torch.ones(EMBED_VOCAB, dtype=torch.bool)
    unused[c["ids"].unique()] = False
    assert unused.any() and (runs[0]["d_word"].cpu()[unused] == 3.0).all()


# ---- 1e: two calls into the same buffers ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("typed", [False, True])
def test_two_calls_accumulate(gpu_device, typed):
    hidden, lens = EMBED_CASES[0]
    c1, ref1 = embed_cases_case(hidden, lens, typed)
    c2 = dict(c1, dy=rng_f16(77, sum(lens), hidden))
    ref2 = reference(c2, typed)
    results = []
    for _ in range(2):
        status, out = raw_call(gpu_device, c1, typed)
        assert status == 0
        status, out = raw_call(gpu_device, c2, typed, out=out)
        assert status == 0
        results.append(out)
    for k in OUTPUTS:
        assert torch.equal(bits(results[0][k]), bits(results[1][k])), k
    check_d_word(results[0]["d_word"], ref1["d_word"] + ref2["d_word"], typed, "two calls")


# ---- 1f: edges -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("typed", [False, True])
def test_one_token(gpu_device, typed):
    c = make_case(1, 128, (1,), EMBED_VOCAB, positions=4)
    got, atomic = run(gpu_device, c, typed), run(gpu_device, c, typed, deterministic=False)
    for k in OUTPUTS:
        assert torch.equal(bits(got[k]), bits(atomic[k])), k
    check_d_word(got["d_word"], reference(c, typed)["d_word"], typed, "one token")


@pytest.mark.parametrize("typed", [False, True])
def test_ids_outside_the_vocabulary_and_garbage_past_the_lengths(gpu_device, typed):
    hidden, lens = EMBED_CASES[0]
    c, _ = embed_cases_case(hidden, lens, typed)
    clean = c["ids"].clone()
    clean[0, 3] = clean[2, 5] = clean[5, 0] = 0
    outside = clean.clone()
    outside[0, 3], outside[2, 5], outside[5, 0] = EMBED_VOCAB, -1, 2 ** 40
    want = run(gpu_device, dict(c, ids=clean), typed)
    got = run(gpu_device, dict(c, ids=outside), typed)
    for k in OUTPUTS:
        assert torch.equal(bits(got[k]), bits(want[k])), k
    garbage = clean.clone()
    pad = torch.arange(max(lens))[None] >= torch.tensor(lens)[:, None]
    garbage[pad] = torch.tensor([-7, 2 ** 40, -2 ** 40, 2 ** 31 + 1]).repeat(int(pad.sum()) // 4 + 1)[:int(pad.sum())]
    got = run(gpu_device, dict(c, ids=garbage), typed)
    for k in OUTPUTS:
        assert torch.equal(bits(got[k]), bits(want[k])), k
    assert (got["d_word"][EMBED_USED:] == 0).all()


@pytest.mark.parametrize("hidden,lens", EMBED_CASES)
def test_null_type_ids_gives_the_untyped_bits(gpu_device, hidden, lens):
    c, _ = embed_cases_case(hidden, lens, True)
    typed = run(gpu_device, dict(c, type_ids=None), True)
    untyped = run(gpu_device, c, False)
    for k in ("dgamma", "dbeta", "d_word", "d_pos"):
        assert torch.equal(bits(typed[k]), bits(untyped[k])), k
    assert torch.equal(bits(typed["d_types"][0]), bits(untyped["d_types"]))
    assert (typed["d_types"][1] == 0).all()


# ---- 1g: non-finite and scaled dy ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("typed", [False, True])
def test_inf_and_nan_reach_the_rows_of_their_ids_only(gpu_device, typed):
    hidden, lens = EMBED_CASES[0]
    c, _ = embed_cases_case(hidden, lens, typed)
    clean = run(gpu_device, c, typed)
    dy = c["dy"].clone()
    t_inf, t_nan = 5, lens[0] + 20                            # tokens (0, 5) and (1, 20)
    dy[t_inf, 3], dy[t_nan, 100] = float("inf"), float("nan")
    hit = {int(c["ids"][0, 5]), int(c["ids"][1, 20])}
    got = run(gpu_device, dict(c, dy=dy), typed)
    rest = torch.ones(EMBED_VOCAB, dtype=torch.bool)
    for k in hit:
        assert not torch.isfinite(got["d_word"][k]).any(), k
        rest[k] = False
    rest = rest.to(gpu_device)
    assert torch.equal(bits(got["d_word"][rest]), bits(clean["d_word"][rest]))
    after = run(gpu_device, c, typed)
    for k in OUTPUTS:
        assert torch.equal(bits(after[k]), bits(clean[k])), k


@pytest.mark.parametrize("typed", [False, True])
def test_a_power_of_two_scales_every_output_exactly(gpu_device, typed):
    hidden, lens = EMBED_CASES[0]
    c, _ = embed_cases_case(hidden, lens, typed)
    small = (c["dy"].float().clamp(-3.0, 3.0) / 4.0).half()
    big = (small.float() * 65536.0).half()
    assert torch.isfinite(big).all() and torch.equal(big.float(), small.float() * 65536.0)
    got, scaled = run(gpu_device, dict(c, dy=small), typed), run(gpu_device, dict(c, dy=big), typed)
    for k in OUTPUTS:
        assert torch.equal(bits(scaled[k]), bits(got[k] * 65536.0)), k


# ---- 1h: refusals --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("typed", [False, True])
def test_refuses_what_it_cannot_run(gpu_device, typed):
    from proqa_amd import _lib
    lib = _lib.load()
    hidden, lens = EMBED_CASES[0]
    c, _ = embed_cases_case(hidden, lens, typed)
    need = lib.proqa_embed_layernorm_backward_det_workspace_bytes(sum(lens), hidden, int(typed))
    refused = [dict(ws_bytes=need - 1), dict(hidden=100), dict(hidden=1032), dict(seq_len=513)]
    refused += [dict(null=name) for name in ("dy", "ids", "cu", "word", "pos", "types", "gamma", "dgamma", "dbeta", "d_word",
                                             "d_pos", "d_types", "ws")]
    if typed:
        refused += [dict(n_types=3)]
    for kw in refused:
        status, out = raw_call(gpu_device, c, typed, fill=7.0, **kw)
        assert status == EINVAL, (kw, status, lib.proqa_last_error())
        assert all((v == 7.0).all() for v in out.values()), kw
    status, out = raw_call(gpu_device, c, typed, fill=7.0)          # and the same call, unrefused
    assert status == 0 and (out["dgamma"] != 7.0).any()
    if typed:
        status, _ = raw_call(gpu_device, c, typed, null="type_ids")
        assert status == 0
