"""proqa_reader_loss_multi_f16 / proqa_reader_loss_multi_backward_f16 and proqa_amd.reader_loss.reader_loss_multi.

The multi-question call is defined by the single-question entry points, bit for bit (include/proqa_hip.h), and those are
held to float64 by tests/test_reader_loss_gpu.py.  So the oracle here is the single-question call on every question's
slice of the operands: rows cu[first sequence] .. cu[last sequence + 1] of hidden, cu_seqlens rebased to 0, the question's
rows of para_embed / labels, q[i], grad_in[i].  Every per-question output must carry the slice call's bits; d_qa_w / d_qa_b
must carry the bits of the slice calls' values added in ascending question order by plain fp32 additions, the slice calls
made at the pack's seq_len (seq_len fixes the number of slabs the compensated sum runs over).

All questions share H = 128, A = 3 and one qa_w / qa_b.  Their geometries are those of tests/test_reader_loss_gpu.py: RAGGED
(lengths on both sides of the 32-row block, an empty paragraph, a sequence without a valid pair) at 300, 65, 64 and 6 = B
passages (both sides of the 64-row rank block, and P = B), ONEROW at 3 passages, one sequence without any valid pair, and
a question whose labels are all 0.

Dropout (p = 0.1) is the one place where a slice call differs (the mask coordinate is the row of the whole pack), so there
the oracle is reader_loss_oracle.evaluate per question with `keep` from proqa_dropout_keep_host at the pack's rows.  The
questions have the shapes of the "dropout" case of tests/test_reader_loss_gpu.py and its bounds hold per question: four
times that row of its table.  d_qa_w / d_qa_b exist for the pack only; each question's part is within its bound
4 E max|ref_i| (max|operand| where the float64 value vanishes by cancellation: that file's rule), so their sum is within
the sum of these of the float64 sum (the Q - 1 fp32 additions add at most Q 2^-24 of the same magnitudes, which the test
adds to the bound).
"""
import ctypes
import functools

import pytest
import torch

import reader_loss_oracle as oracle
from test_reader_loss_gpu import CALL, CANCEL, ONEROW, RAGGED, REFERENCE_ERROR, SEED, SITE, VARIANTS, errors

pytestmark = pytest.mark.gpu

H, A = 128, 3
NOPAIR = dict(lens=[20], para_offset=[5], start=[[-1, 3, -1]], end=[[-1, 30, -1]])       # (3, 30) lies outside the mask
TWO = dict(lens=[33, 12], para_offset=[9, 7], start=[[9, 3, -1], [8, 10, -1]], end=[[31, 10, -1], [10, 11, -1]])
QUESTIONS = {
    # name: geometry, passages, labels are set
    "ragged300": (RAGGED, 300, True),
    "ragged65": (RAGGED, 65, True),
    "ragged64": (RAGGED, 64, True),
    "p_equals_b": (RAGGED, 6, True),
    "onerow": (ONEROW, 3, True),
    "nopair": (NOPAIR, 64, True),
    "nogold": (TWO, 65, False),
}
PACKS = {
    "q1": ["ragged300"],
    "q2": ["ragged300", "onerow"],
    "q2_reversed": ["onerow", "ragged300"],
    "q3": ["nopair", "ragged65", "nogold"],
    "q3_reversed": ["nogold", "ragged65", "nopair"],
    "q5": ["ragged300", "onerow", "nopair", "p_equals_b", "ragged64"],
    "q5_reversed": ["ragged64", "p_equals_b", "nopair", "onerow", "ragged300"],
}
GRADS = (1.0, 1024.0, 0.25)
DTYPES = [torch.float16, torch.float32]
KEYS = ("loss_out", "logits", "stats", "d_hidden", "d_q")


@functools.lru_cache(maxsize=None)
def weights():
    g = torch.Generator().manual_seed(11)
    return (0.3 * torch.randn(2, H, generator=g)).half(), (0.1 * torch.randn(2, generator=g)).half()


@functools.lru_cache(maxsize=None)
def make_question(name, seed_offset=0):
    """One question on the CPU: packed hidden [T_i, H] and the rest, para in fp32 (cast by the pack)."""
    geo, P, gold = QUESTIONS[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + seed_offset)
    lens = geo["lens"]
    labels = torch.zeros(P, dtype=torch.int64)
    if gold:
        labels[[0, P // 2, P - 1]] = 1
    return dict(lens=lens, hidden=torch.randn(sum(lens), H, generator=g).half(), para=0.4 * torch.randn(P, 128, generator=g),
                labels=labels, q=(0.4 * torch.randn(128, generator=g)).half(), start=torch.tensor(geo["start"]),
                end=torch.tensor(geo["end"]), para_offset=torch.tensor(geo["para_offset"]))


def make_pack(questions, dtype):
    """The operands of the multi call on the CPU, and the questions' slices of them."""
    lens = [n for c in questions for n in c["lens"]]
    seq, para, rows = [0], [0], [0]
    for c in questions:
        seq.append(seq[-1] + len(c["lens"]))
        para.append(para[-1] + c["para"].shape[0])
        rows.append(rows[-1] + sum(c["lens"]))
    cat = lambda k: torch.cat([c[k] for c in questions])
    return dict(hidden=cat("hidden"), para=cat("para").to(dtype), labels=cat("labels"), q=torch.stack([c["q"] for c in questions]),
                start=cat("start"), end=cat("end"), para_offset=cat("para_offset"), lens=lens, seq=seq, paras=para, rows=rows,
                cu=torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32), seq_len=max(lens),
                grad=torch.tensor([GRADS[i % len(GRADS)] for i in range(len(questions))], dtype=torch.float32))


def slice_of(pack, i):
    """Question i's operands cut out of the pack: what the single-question call is given."""
    b0, b1, p0, p1, r0, r1 = *pack["seq"][i:i + 2], *pack["paras"][i:i + 2], *pack["rows"][i:i + 2]
    return dict(hidden=pack["hidden"][r0:r1], para=pack["para"][p0:p1], labels=pack["labels"][p0:p1], q=pack["q"][i],
                start=pack["start"][b0:b1], end=pack["end"][b0:b1], para_offset=pack["para_offset"][b0:b1],
                cu=pack["cu"][b0:b1 + 1] - pack["cu"][b0], seq_len=pack["seq_len"], grad=pack["grad"][i:i + 1])


def run_multi(pack, dev, shared_norm=True, early=True, p=0.0, device_csr=False):
    from proqa_amd import reader_loss as RL
    to = lambda k: pack[k].to(dev)
    hidden = to("hidden").contiguous()
    seq, paras = pack["seq"], pack["paras"]
    extra = {}
    if device_csr:
        extra = dict(max_seqs=max(b - a for a, b in zip(seq, seq[1:])), max_paras=max(b - a for a, b in zip(paras, paras[1:])))
        seq, paras = torch.tensor(seq, device=dev), torch.tensor(paras, device=dev)
    geo = RL._MultiGeometry(hidden, len(pack["seq"]) - 1, to("cu"), seq, paras, extra.get("max_seqs"), extra.get("max_paras"),
                            to("para_offset"), to("start"), to("end"), to("para"), to("labels"), shared_norm, early, p,
                            (SEED, CALL), pack["seq_len"])
    w16, b16 = (t.to(dev) for t in weights())
    q = to("q").contiguous()
    loss_out, logits, stats = RL.reader_loss_multi_forward(hidden, w16, b16, q, geo)
    d_hidden, d_w, d_b, d_q = RL.reader_loss_multi_backward(hidden, w16, q, geo, logits, stats, to("grad"))
    return dict(loss_out=loss_out.cpu(), logits=logits.cpu(), stats=stats.cpu(), d_hidden=d_hidden.cpu(), d_qa_w=d_w.cpu(),
                d_qa_b=d_b.cpu(), d_q=d_q.cpu())


def run_single(s, dev, shared_norm=True, early=True):
    from proqa_amd import reader_loss as RL
    to = lambda k: s[k].to(dev)
    hidden = to("hidden").contiguous()
    geo = RL._Geometry(hidden, to("cu"), None, to("para_offset"), to("start"), to("end"), to("para").contiguous(), to("labels"),
                       shared_norm, early, 0.0, None, s["seq_len"])
    w16, b16 = (t.to(dev) for t in weights())
    q = to("q").contiguous()
    loss_out, logits, stats = RL.reader_loss_forward(hidden, w16, b16, q, geo)
    d_hidden, d_w, d_b, d_q = RL.reader_loss_backward(hidden, w16, q, geo, logits, stats, to("grad"))
    return dict(loss_out=loss_out.cpu(), logits=logits.cpu(), stats=stats.cpu(), d_hidden=d_hidden.cpu(), d_qa_w=d_w.cpu(),
                d_qa_b=d_b.cpu(), d_q=d_q.cpu())


def part_of(pack, got, i):
    """Question i's part of the multi call's per-question outputs, shaped like the single call's."""
    b0, r0, r1 = pack["seq"][i], *pack["rows"][i:i + 2]
    n = 8 + 2 * (pack["seq"][i + 1] - b0)
    return dict(loss_out=got["loss_out"][i], logits=got["logits"][r0:r1], stats=got["stats"][8 * i + 2 * b0:8 * i + 2 * b0 + n],
                d_hidden=got["d_hidden"][r0:r1], d_q=got["d_q"][i])


def bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.float16 else torch.int32)


def assert_same_bits(a, b, keys, what):
    for k in keys:
        assert a[k].shape == b[k].shape and torch.equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"


# ---- the contract: the bits of the slice calls -------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["para16", "para32"])
@pytest.mark.parametrize("pack_name", list(PACKS))
def test_bits_of_the_slice_calls(gpu_device, pack_name, dtype):
    pack = make_pack([make_question(n) for n in PACKS[pack_name]], dtype)
    n_q = len(PACKS[pack_name])
    for shared_norm, early in VARIANTS:
        what = f"{pack_name} norm={shared_norm} early={early}"
        got = run_multi(pack, gpu_device, shared_norm, early)
        singles = [run_single(slice_of(pack, i), gpu_device, shared_norm, early) for i in range(n_q)]
        for i in range(n_q):
            assert_same_bits(part_of(pack, got, i), singles[i], KEYS, f"{what} question {i}")
        # d_qa_w / d_qa_b: ((v_0 + v_1) + v_2) + ... in fp32
        for k in ("d_qa_w", "d_qa_b"):
            want = singles[0][k].clone()
            for s in singles[1:]:
                want = want + s[k]
            assert torch.equal(bits(got[k]), bits(want)), f"{what}: {k} is not the ascending fp32 sum"
        assert torch.isfinite(got["loss_out"]).all()
        assert_same_bits(got, run_multi(pack, gpu_device, shared_norm, early), KEYS + ("d_qa_w", "d_qa_b"), f"{what} second run")
    # the CSR arrays given on the device (nothing checked on the host) are the same call
    assert_same_bits(got, run_multi(pack, gpu_device, *VARIANTS[-1], device_csr=True), KEYS + ("d_qa_w", "d_qa_b"), "device CSR")


def test_linear_in_each_questions_gradient(gpu_device):
    pack = make_pack([make_question(n) for n in PACKS["q3"][1:] + ["ragged300"]], torch.float16)
    ones = dict(pack, grad=torch.ones(3))
    one, got = run_multi(ones, gpu_device), run_multi(pack, gpu_device)
    assert tuple(pack["grad"].tolist()) == GRADS
    assert_same_bits(one, got, ("loss_out", "logits", "stats"), "forward")
    for i, k in enumerate(GRADS):
        a, b = part_of(pack, one, i), part_of(pack, got, i)
        for name in ("d_hidden", "d_q"):
            x, y = a[name].float().flatten(), b[name].float().flatten()
            normal = (x.abs() >= 2.0 ** -14) & ((x * k).abs() >= 2.0 ** -14)      # fp16 normal before and after
            assert normal.any() and torch.equal(y[normal], x[normal] * k), f"question {i} {name} x {k}"
            assert ((y - x * k).abs() <= max(k, 1.0) * 2.0 ** -24).all(), f"question {i} {name} x {k}"   # (fp16's subnormal step)


def test_no_reads_across_questions(gpu_device):
    names = ["ragged65", "nogold", "onerow"]
    clean_q = [make_question(n) for n in names]
    clean = make_pack(clean_q, torch.float32)
    ref = run_multi(clean, gpu_device)
    for j in range(3):
        bad = dict(clean_q[j])
        bad["hidden"] = torch.full_like(bad["hidden"], float("nan"))
        bad["para"] = torch.full_like(bad["para"], float("nan"))
        bad["labels"] = torch.full_like(bad["labels"], 1) - clean_q[j]["labels"]
        bad["q"] = torch.full_like(bad["q"], float("nan"))
        pack = make_pack(clean_q[:j] + [bad] + clean_q[j + 1:], torch.float32)
        got = run_multi(pack, gpu_device)
        assert not torch.isfinite(got["loss_out"][j, 0])
        for i in range(3):
            if i != j:
                assert_same_bits(part_of(pack, got, i), part_of(clean, ref, i), KEYS, f"question {i} beside a NaN question {j}")


def test_device_arrays_that_leave_a_question_empty(gpu_device):
    """Device CSR arrays cannot be checked without a read-back (include/proqa_hip.h): a question they leave without a
    sequence gets a zero loss and no gradient, and the well-formed questions beside it keep their bits."""
    from proqa_amd import reader_loss as RL
    dev = gpu_device
    pack = make_pack([make_question("ragged65"), make_question("nogold")], torch.float16)
    want = run_multi(pack, dev)
    seq = torch.tensor([0, 6, 6, 8], device=dev)            # question 1 of 3 owns nothing
    paras = torch.tensor([0, 65, 65, 130], device=dev)
    to = lambda k: pack[k].to(dev)
    hidden = to("hidden").contiguous()
    geo = RL._MultiGeometry(hidden, 3, to("cu"), seq, paras, 6, 65, to("para_offset"), to("start"), to("end"), to("para"),
                            to("labels"), True, True, 0.0, None, pack["seq_len"])
    w16, b16 = (t.to(dev) for t in weights())
    q = torch.stack([pack["q"][0], torch.full((128,), float("nan"), dtype=torch.float16), pack["q"][1]]).to(dev)
    grad = torch.tensor([GRADS[0], 7.0, GRADS[1]], device=dev)
    loss_out, logits, stats = RL.reader_loss_multi_forward(hidden, w16, b16, q, geo)
    d_hidden, d_w, d_b, d_q = RL.reader_loss_multi_backward(hidden, w16, q, geo, logits, stats, grad)
    assert torch.equal(loss_out[[0, 2]].cpu(), want["loss_out"]) and (loss_out[1] == 0).all()
    assert torch.equal(bits(logits.cpu()), bits(want["logits"])) and torch.equal(bits(d_hidden.cpu()), bits(want["d_hidden"]))
    assert torch.equal(bits(d_q[[0, 2]].cpu()), bits(want["d_q"])) and (d_q[1] == 0).all()
    assert torch.equal(bits(d_w.cpu()), bits(want["d_qa_w"])) and torch.equal(bits(d_b.cpu()), bits(want["d_qa_b"]))


# ---- dropout: the mask is the pack's ----------------------------------------------------------------------------------------

def pack_keep(p, pack, i, L):
    """[B_i, L, H] bool: proqa_dropout_keep_host at (row of the WHOLE pack, column), site 255"""
    from proqa_amd import _lib
    lib = _lib.load()
    lens = pack["lens"][pack["seq"][i]:pack["seq"][i + 1]]
    keep = torch.zeros((len(lens), L, H), dtype=torch.bool)
    buf = (ctypes.c_uint8 * H)()
    row = pack["rows"][i]
    for b, n in enumerate(lens):
        for t in range(n):
            _lib.check(lib.proqa_dropout_keep_host(0, p, SEED, SITE, CALL, row, 0, 0, H, buf))
            keep[b, t] = torch.tensor(list(buf), dtype=torch.bool)
            row += 1
    return keep


def padded(x, lens, L):
    out = torch.zeros((len(lens), L) + tuple(x.shape[1:]), dtype=x.dtype)
    row = 0
    for b, n in enumerate(lens):
        out[b, :n] = x[row:row + n]
        row += n
    return out


def test_dropout_against_float64_per_question(gpu_device):
    import math
    p = 0.1
    questions = [make_question("ragged300", seed_offset=k) for k in range(3)]
    pack = dict(make_pack(questions, torch.float16), grad=torch.ones(3))
    qa_w, qa_b = weights()
    thr = min(65535, math.floor(p * 65536 + 0.5))
    factor = float(torch.tensor(1.0, dtype=torch.float32) / (1.0 - torch.tensor(thr / 65536.0, dtype=torch.float32)))
    L = pack["seq_len"]
    cases = []
    for i in range(3):
        s = slice_of(pack, i)
        lens = questions[i]["lens"]
        cases.append(dict(hidden=padded(s["hidden"], lens, L), qa_w=qa_w, qa_b=qa_b, q=s["q"], para=s["para"], labels=s["labels"],
                          start=s["start"], end=s["end"], lens=lens, para_offset=s["para_offset"].tolist(),
                          keep=pack_keep(p, pack, i, L), factor=factor))
    assert not torch.equal(cases[0]["keep"], cases[1]["keep"])          # the questions' masks are independent
    bound = {k: 4.0 * v for k, v in REFERENCE_ERROR["dropout"].items()}
    for shared_norm, early in VARIANTS:
        got = run_multi(pack, gpu_device, shared_norm, early, p=p)
        refs = [oracle.evaluate(**c, shared_norm=shared_norm, early=early) for c in cases]
        for i, (c, ref) in enumerate(zip(cases, refs)):
            part = part_of(pack, got, i)
            mine = dict(loss=part["loss_out"][0], logits=padded(part["logits"], c["lens"], L),
                        d_hidden=padded(part["d_hidden"], c["lens"], L), d_q=part["d_q"], d_qa_w=ref["d_qa_w"], d_qa_b=ref["d_qa_b"])
            errs = errors(c, mine, ref)
            for k in ("loss", "logits", "d_hidden", "d_q"):
                print(f"dropout norm={shared_norm} early={early} question {i} {k}: error {errs[k]:.3e} bound {bound[k]:.3e}")
                assert errs[k] <= bound[k], f"question {i} {k}: error {errs[k]:.3e} over {bound[k]:.3e}"
        for k in ("d_qa_w", "d_qa_b"):
            total = sum(r[k] for r in refs)
            # (a sum that vanishes by cancellation is measured against its operands: the rule of test_reader_loss_gpu.py)
            operand = {"d_qa_w": [float(c["hidden"].abs().max()) for c in cases], "d_qa_b": [1.0] * 3}[k]
            tops = [float(r[k].abs().max()) for r in refs]
            room = sum(top if top >= CANCEL * op else op for top, op in zip(tops, operand))
            err = float((got[k].double() - total).abs().max())
            limit = (bound[k] + 3 * 2.0 ** -24) * room
            print(f"dropout norm={shared_norm} early={early} {k}: |error| {err:.3e} bound {limit:.3e}")
            assert err <= limit, f"{k}: |error| {err:.3e} over {limit:.3e}"
    # the mask of the pack: d_hidden is zero exactly where the element was dropped (a gradient of 2^12 keeps the small ones)
    big = run_multi(dict(pack, grad=torch.full((3,), 4096.0)), gpu_device, p=p)
    for i, c in enumerate(cases):
        mask = oracle._mask(L, c["lens"], c["para_offset"])
        d = padded(part_of(pack, big, i)["d_hidden"], c["lens"], L)
        assert torch.equal(d[mask] != 0, c["keep"][mask]), f"question {i}"


# ---- the Python entry point ---------------------------------------------------------------------------------------------------

def test_reader_loss_multi_is_one_node_without_a_host_wait(gpu_device):
    from proqa_amd.reader_loss import reader_loss, reader_loss_multi
    pack = make_pack([make_question(n) for n in PACKS["q3"]], torch.float16)
    dev = gpu_device
    w16, b16 = weights()

    def leaves():
        return (pack["hidden"].to(dev).requires_grad_(True), w16.float().to(dev).requires_grad_(True),
                b16.float().to(dev).requires_grad_(True), pack["q"].to(dev).requires_grad_(True))
    rest = dict(para_embed=pack["para"].to(dev), top5000_labels=pack["labels"].to(dev), start_positions=pack["start"].to(dev),
                end_positions=pack["end"].to(dev), para_offset=pack["para_offset"].to(dev), cu_seqlens=pack["cu"].to(dev),
                question_seq=pack["seq"], question_para=pack["paras"], max_seq_len=pack["seq_len"])
    weight = pack["grad"].to(dev)
    hidden, w, b, q = leaves()
    (reader_loss_multi(hidden, w, b, q, **rest)["losses"] * weight).sum().backward()      # (the workspace is allocated here)
    hidden, w, b, q = leaves()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = reader_loss_multi(hidden, w, b, q, **rest)
        (out["losses"] * weight).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out["losses"].shape == (3,) and out["joint"].shape == (3,) and not out["early"].requires_grad
    assert out["losses"].grad_fn.next_functions[0][0].name().startswith("_ReaderLoss")
    low = run_multi(pack, dev)
    assert torch.equal(hidden.grad.cpu(), low["d_hidden"]) and torch.equal(q.grad.cpu(), low["d_q"])
    assert torch.equal(w.grad.cpu(), low["d_qa_w"]) and torch.equal(b.grad.cpu(), low["d_qa_b"])
    assert torch.equal(out["losses"].detach().cpu(), low["loss_out"][:, 0])
    assert torch.equal(out["joint"].cpu(), low["loss_out"][:, 1]) and torch.equal(out["early"].cpu(), low["loss_out"][:, 2])
    # reader_loss on the first question alone: the same loss bits
    s = slice_of(pack, 0)
    alone = reader_loss(s["hidden"].to(dev), w.detach(), b.detach(), s["q"].to(dev), s["para"].to(dev), s["labels"].to(dev),
                        s["start"].to(dev), s["end"].to(dev), s["para_offset"].to(dev), cu_seqlens=s["cu"].to(dev),
                        max_seq_len=pack["seq_len"])
    assert alone["loss"].item() == out["losses"][0].item()
    with pytest.raises(ValueError):
        reader_loss_multi(hidden, w, b, q, **dict(rest, question_seq=pack["seq"][:-1]))
    with pytest.raises(ValueError):
        reader_loss_multi(hidden, w, b, q, **dict(rest, question_seq=torch.tensor(pack["seq"], device=dev)))


# ---- refusals, before the device is touched ----------------------------------------------------------------------------------

def test_refusals_before_the_device_is_touched(gpu_device):
    from proqa_amd import _lib
    lib = _lib.load()
    csr = lambda v: (ctypes.c_int32 * len(v))(*v)
    ok = dict(hidden=4096, cu=4096, batch=7, seq_len=40, hsize=H, para_offset=4096, qa_w=4096, qa_b=4096, start=4096, end=4096,
              n_answers=A, q=4096, para=4096, dtype=_lib.PROQA_F16, labels=4096, n_paras=303, dim=128, seq_dev=4096,
              para_dev=4096, n_q=2, max_seqs=6, max_paras=300, seq_host=csr([0, 6, 7]), para_host=csr([0, 300, 303]), flags=1,
              p=0.0, seed=0, site=255, call=0, logits=4096, stats=4096, loss=4096, ws=4096, ws_bytes=1 << 30, stream=None)

    def forward(**changes):
        a = dict(ok, **changes)
        return lib.proqa_reader_loss_multi_f16(*a.values())

    def backward(**changes):
        a = dict(ok, **changes)
        for k in ("qa_b", "loss"):
            del a[k]
        items = list(a.items())
        at = [k for k, _ in items].index("stats") + 1
        items[at:at] = [("grad_in", 4096), ("d_hidden", 4096), ("d_qa_w", 4096), ("d_qa_b", 4096), ("d_q", 4096)]
        return lib.proqa_reader_loss_multi_backward_f16(*[v for _, v in items])

    refused = {
        "no question": dict(n_q=0),
        "more paragraphs' sequences than rows (P_i < B_i)": dict(seq_host=csr([0, 3, 7]), para_host=csr([0, 300, 303])),
        "an empty question": dict(seq_host=csr([0, 7, 7]), max_seqs=7),
        "CSR that does not cover": dict(seq_host=csr([0, 6, 6])),
        "one host array alone": dict(para_host=None),
        "misaligned hidden": dict(hidden=4104),
        "misaligned q": dict(q=4098),
        "misaligned para_embed": dict(para=4100),
        "too many questions": dict(n_q=4097, batch=5000, n_paras=5000, seq_host=None, para_host=None, max_seqs=2, max_paras=2),
        "too many sequences": dict(batch=65537, n_paras=65537 + 296, seq_host=None, para_host=None, max_seqs=65536, max_paras=65536),
        "too many rows of para_embed": dict(n_paras=(1 << 22) + 1, seq_host=None, para_host=None, max_paras=65536),
        "a question over 65536 rows": dict(n_paras=70000, seq_host=None, para_host=None, max_paras=65537),
        "max_paras too small for P": dict(seq_host=None, para_host=None, max_paras=151),
        "sequence too long": dict(seq_len=4097),
        "hidden not a multiple of 8": dict(hsize=100),
        "dim": dict(dim=64),
    }
    for what, changes in refused.items():
        for call in (forward, backward):
            assert call(**changes) == -1, what         # PROQA_EINVAL
            assert lib.proqa_last_error(), what
    assert lib.proqa_reader_loss_multi_workspace_bytes(0, 7, 40, H, A, 303, 300) == 0
    need = lib.proqa_reader_loss_multi_workspace_bytes(2, 7, 40, H, A, 303, 300)
    assert need > 0 and forward(ws_bytes=need - 16) == -1
    # and the same sizes with one question are the single call's workspace
    assert lib.proqa_reader_loss_multi_workspace_bytes(1, 6, 40, H, A, 300, 300) == lib.proqa_reader_loss_workspace_bytes(6, 40, H, A, 300)
