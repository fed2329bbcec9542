"""proqa_inbatch_eval_f16 and `train_retriever.py --do_predict` on the GPU, against tests/inbatch_oracle.py (NumPy float64)
on the kernel's own inputs.

Tolerances (none of them measured on the kernel):
  max / gold   fp32 accumulation bound 128 * 2^-24 * sum_d |q_d c_d| of that (question, column) pair
               (inbatch_oracle.accumulation_bound): gold against the bound of its target column, max against the bound of
               the oracle's argmax column on the rows the oracle decides (on an undecided row the device may hold another
               column's score: there the row's greatest bound).  Integer-valued inputs are exact: the bits are compared.
  argmax/rank  equal on every row the float64 oracle decides by more than twice that bound; at most 5 % of the rows may
               be undecided, and the seeds below leave none (checked on the CPU in tests/test_retriever_eval_host.py).
  lse          score bound + (nc + K_INTRINSICS) * 2^-24 + 2^-23 * |lse|.  The first term is the error of the scores
               (log-sum-exp is 1-Lipschitz in the max norm), nc * 2^-24 the fp32 summation of nc terms in (0, 1], the last
               the rounding of log(sum) + max to fp32.  K_INTRINSICS allows for exp / log: the reference's own
               arithmetic, torch.log_softmax in fp32 on the CPU, is off the float64 value of the same fp32 scores by at
               most 54.4 * 2^-24 over the lse cases of this file (measure_reference_lse_error, run on the CPU);
               device intrinsics are looser than libm, so 4 x that, rounded up first: K_INTRINSICS = 4 * 55 = 220.
"""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import inbatch_oracle as oracle

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

K_INTRINSICS = 220
U = 2.0 ** -24
MAX_UNDECIDED = 0.05

GAUSSIAN_SHAPES = [(100, 100), (300, 777)]
GAUSSIAN_SEEDS = {(100, 100): 0, (300, 777): 8}      # the first seeds that leave no undecided row


# ---- inputs (pure NumPy: the host test imports these) ------------------------------------------------------------------

def gaussian_case(nq, nc):
    """N(0, 1) fp16 paragraphs; question i is N(0, 1) + c[target_i] / 4, so its gold scores about 32 among scores of
    standard deviation 11: a handful of columns beat it (ranks are not trivial) and few sit within 1e-3 of it.  (100, 100)
    uses the implicit target i, (300, 777) an explicit random one."""
    rng = np.random.default_rng(GAUSSIAN_SEEDS[(nq, nc)])
    c = rng.standard_normal((nc, 128)).astype(np.float16)
    target = None if nq == nc else rng.integers(0, nc, nq).astype(np.int32)
    t = np.arange(nq) if target is None else target
    q = (rng.standard_normal((nq, 128)) + 0.25 * c[t].astype(np.float64)).astype(np.float16)
    return q, c, target


def decided_rows(q, c, target):
    """(rows whose argmax, rows whose rank the float64 oracle decides by more than twice the accumulation bound, bound)."""
    o = oracle.inbatch_eval(q, c, target)
    s = o["scores"]
    bound = oracle.accumulation_bound(q, c).max(1)
    top = np.sort(s, 1)
    margin = top[:, -1] - top[:, -2] if s.shape[1] > 1 else np.full(len(s), np.inf)
    others = np.abs(s - o["gold"][:, None])
    others[np.arange(len(s)), o["target"]] = np.inf
    return margin > 2 * bound, others.min(1) > 2 * bound, bound


def magnitude_case():
    """(33, 65) with entries of magnitude about 15: golds near +3e4, and the negated paragraphs near -3e4.  exp(3e4)
    overflows fp32 (and float64): without the maximum subtracted every lse is inf."""
    rng = np.random.default_rng(5)
    c = (rng.choice([-1.0, 1.0], (65, 128)) * (15.0 + rng.uniform(-0.5, 0.5, (65, 128)))).astype(np.float16)
    c[33:] = -c[:32]
    q = c[:33].copy()
    return q, c, None


TIE_COLUMNS = (31, 33, 511, 512)


def integer_case(nq, nc, seed):
    """Integer-valued fp16 in [-4, 4]: every product and partial sum is an integer below 2^24, exact in fp32 whatever the
    order.  Golds in column 0, column nc - 1 and the first column of the last (partial) 32-column tile; rows 0 .. 3 ask
    about their gold paragraph itself (the gold is then the row's greatest score).  Row 3's gold is column 32, the first of
    the second tile, and the same paragraph also sits at column 31 (left of the gold, in the tile before), 33, and 511 /
    512 (column 512 starts the second workgroup split of both split shapes): its greatest score is tied across a tile
    boundary and a split boundary, on both sides of the gold."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-4, 5, (nq, 128)).astype(np.float16)
    c = rng.integers(-4, 5, (nc, 128)).astype(np.float16)
    target = rng.integers(0, nc, nq).astype(np.int32)
    fixed = [0, nc - 1, (nc - 1) // 32 * 32, min(nc - 1, 32)]
    for r, t in enumerate(fixed[:nq]):
        target[r] = t
    if nq > 3:
        for col in TIE_COLUMNS:
            if col < nc:
                c[col] = c[target[3]]
    for r in range(min(nq, 4)):
        q[r] = c[target[r]]
    return q, c, target


def measure_reference_lse_error():
    """max |torch fp32 (lse - gold) - float64 (lse - gold)| / 2^-24 on the fp32-rounded scores of the lse cases: the error
    of -log_softmax(product)[i, target_i], the reference's CrossEntropyLoss term.  CPU only; gives K_INTRINSICS / 4."""
    worst = 0.0
    for q, c, target in [gaussian_case(*s) for s in GAUSSIAN_SHAPES] + [magnitude_case()]:
        s32 = oracle.scores(q, c).astype(np.float32)
        t = np.arange(len(q)) if target is None else target
        ref = -torch.log_softmax(torch.from_numpy(s32), -1).numpy()[np.arange(len(q)), t]
        exact = oracle.logsumexp(s32) - s32.astype(np.float64)[np.arange(len(q)), t]
        worst = max(worst, float((np.abs(ref - exact) / U).max()))
    return worst


# ---- helpers -------------------------------------------------------------------------------------------------------------

def run(dev, q, c, target=None):
    from proqa_amd.inbatch import inbatch_eval
    out = inbatch_eval(torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev),
                       None if target is None else torch.from_numpy(target).to(dev))
    assert all(v.is_cuda and v.shape == (len(q),) for v in out.values())
    assert out["argmax"].dtype == out["rank"].dtype == torch.int32
    assert out["max"].dtype == out["gold"].dtype == out["lse"].dtype == torch.float32
    return {k: v.cpu().numpy() for k, v in out.items()}


def lse_tolerance(q, c, want_lse):
    nc = len(c)
    return oracle.accumulation_bound(q, c).max(1) + (nc + K_INTRINSICS) * U + 2.0 ** -23 * np.abs(want_lse)


def pair_bounds(q, c, want, keep_argmax):
    """(bound of max, bound of gold) per row: the accumulation bound of the pair the value belongs to."""
    b = oracle.accumulation_bound(q, c)
    rows = np.arange(len(q))
    return np.where(keep_argmax, b[rows, want["argmax"]], b.max(1)), b[rows, want["target"]]


def check_lse(got, want, tol):
    finite = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~finite & ~np.isnan(want)], want[~finite & ~np.isnan(want)])      # +-inf
    err = np.abs(got[finite].astype(np.float64) - want[finite])
    print("lse: max error", err.max() if err.size else 0.0, "tolerance at that row", tol[finite][err.argmax()] if err.size else 0.0)
    assert (err <= tol[finite]).all()


def check_toleranced(dev, q, c, target):
    got = run(dev, q, c, target)
    want = oracle.inbatch_eval(q, c, target)
    keep_argmax, keep_rank, bound = decided_rows(q, c, target)
    print("undecided rows: argmax", int((~keep_argmax).sum()), "rank", int((~keep_rank).sum()), "of", len(q))
    assert (~keep_argmax).mean() <= MAX_UNDECIDED and (~keep_rank).mean() <= MAX_UNDECIDED
    for key, pair_bound in zip(("max", "gold"), pair_bounds(q, c, want, keep_argmax)):
        err = np.abs(got[key].astype(np.float64) - want[key])
        print(key, "max error", err.max(), "bound of that pair", pair_bound[err.argmax()])
        assert (err <= pair_bound).all()
    assert np.array_equal(got["argmax"][keep_argmax], want["argmax"][keep_argmax])
    assert np.array_equal(got["rank"][keep_rank], want["rank"][keep_rank])
    check_lse(got["lse"], want["lse"], lse_tolerance(q, c, want["lse"]))
    return got, want


# ---- 1: integer-valued embeddings, every output exact --------------------------------------------------------------------

INTEGER_SHAPES = [(1, 1), (1, 100), (33, 65), (100, 100), (257, 1000), (8, 20000)]


@pytest.mark.parametrize("nq,nc", INTEGER_SHAPES)
def test_integer_embeddings_are_exact(gpu_device, nq, nc):
    q, c, target = integer_case(nq, nc, seed=nq * 100003 + nc)
    want = oracle.inbatch_eval(q, c, target)
    s = want["scores"]
    if nq > 3 and nc > 33:      # the planted ties are there: row 3's greatest score at its gold and on both sides of it
        cols = [col for col in TIE_COLUMNS if col < nc]
        assert target[3] == 32 and all(s[3, col] == want["gold"][3] == want["max"][3] for col in cols)
        assert want["argmax"][3] == 31 and want["rank"][3] == 1
        assert (nc <= 512) or {511, 512} <= set(cols)
    got = run(gpu_device, q, c, target)
    assert np.array_equal(got["argmax"], want["argmax"])
    assert np.array_equal(got["rank"], want["rank"])
    for key in ("max", "gold"):
        assert np.array_equal(got[key].view(np.int32), want[key].astype(np.float32).view(np.int32)), key
    check_lse(got["lse"], want["lse"], lse_tolerance(q, c, want["lse"]))
    if nq <= nc:                # the implicit target i
        got = run(gpu_device, q, c, None)
        want = oracle.inbatch_eval(q, c, None)
        assert np.array_equal(got["argmax"], want["argmax"]) and np.array_equal(got["rank"], want["rank"])
        assert np.array_equal(got["gold"].view(np.int32), want["gold"].astype(np.float32).view(np.int32))


# ---- 2 + 3: Gaussian embeddings, and lse ---------------------------------------------------------------------------------

@pytest.mark.parametrize("nq,nc", GAUSSIAN_SHAPES)
def test_gaussian_embeddings_within_the_accumulation_bound(gpu_device, nq, nc):
    q, c, target = gaussian_case(nq, nc)
    got, want = check_toleranced(gpu_device, q, c, target)
    assert 0 < (want["rank"] > 0).sum() < nq        # the case has right and wrong rows


def test_lse_at_scores_near_3e4_needs_the_maximum_subtracted(gpu_device):
    q, c, target = magnitude_case()
    want = oracle.inbatch_eval(q, c, target)
    assert want["scores"].max() > 2.8e4 and want["scores"].min() < -2.8e4
    with np.errstate(over="ignore"):
        assert np.isinf(np.log(np.exp(want["scores"].astype(np.float32)).sum(1))).all()     # the unshifted form fails
    assert np.isfinite(want["lse"]).all()
    check_toleranced(gpu_device, q, c, target)


# ---- 4: non-finite input -----------------------------------------------------------------------------------------------

def test_non_finite_scores_follow_torch(gpu_device):
    """A NaN in question 3 (its whole row is NaN), +inf in element 0 of paragraph 10 (column 10 is +-inf by the sign of
    q[i, 0]), and -inf in element 5 of question 7 against positive c[:, 5] (row 7 is all -inf)."""
    rng = np.random.default_rng(21)
    q = rng.standard_normal((33, 128)).astype(np.float16)
    c = rng.standard_normal((65, 128)).astype(np.float16)
    assert (q != 0).all() and (c != 0).all()
    c[:, 5] = np.abs(c[:, 5])
    q[3, 17] = np.nan
    c[10, 0] = np.inf
    q[7, 5] = -np.inf
    q[7, 0] = -np.abs(q[7, 0])
    want = oracle.inbatch_eval(q, c, None)
    s = want["scores"]
    assert np.isnan(s[3]).all() and np.isneginf(s[7]).all() and np.isinf(np.delete(s, 3, 0)[:, 10]).all()
    assert want["argmax"][3] == 0 and want["rank"][3] == 3 and want["argmax"][7] == 0 and want["rank"][7] == 7
    pos = np.flatnonzero(np.isposinf(s[:, 10]))
    assert len(pos) > 3 and (want["argmax"][pos] == 10).all() and np.isposinf(want["lse"][pos]).all()
    got = run(gpu_device, q, c, None)                   # returns: no fault, no endless loop
    assert np.array_equal(got["argmax"], want["argmax"])
    assert np.array_equal(got["rank"], want["rank"])
    qz, cz = np.nan_to_num(q, posinf=0, neginf=0), np.nan_to_num(c, posinf=0, neginf=0)      # bounds of the finite scores
    bound = oracle.accumulation_bound(qz, cz).max(1)
    # max is finite on the rows whose column 10 is -inf; decided as in check_toleranced, on the finite scores
    top = np.sort(np.where(np.isfinite(s), s, -np.inf), 1)
    with np.errstate(invalid="ignore"):
        keep_argmax = np.isfinite(want["max"]) & (top[:, -1] - top[:, -2] > 2 * bound)
    assert keep_argmax.sum() > 3
    safe_argmax = dict(want, argmax=np.where(keep_argmax, want["argmax"], 0))
    for key, pair_bound in zip(("max", "gold"), pair_bounds(qz, cz, safe_argmax, keep_argmax)):
        finite = np.isfinite(want[key])
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
        assert np.array_equal(got[key][~finite & ~np.isnan(want[key])], want[key][~finite & ~np.isnan(want[key])]), key
        assert (np.abs(got[key][finite] - want[key][finite]) <= pair_bound[finite]).all(), key
    assert np.isnan(got["lse"][3]) and np.isneginf(got["lse"][7])
    check_lse(got["lse"], want["lse"], bound + (65 + K_INTRINSICS) * U + 2.0 ** -23 * np.abs(np.nan_to_num(want["lse"], posinf=0, neginf=0)))


# ---- 5: the C entry point's argument rules -----------------------------------------------------------------------------

def test_null_outputs_empty_batch_and_refusals(gpu_device):
    from proqa_amd import _lib
    lib = _lib.load()
    q, c, target = integer_case(33, 65, seed=9)
    full = run(gpu_device, q, c, target)
    dq, dc = torch.from_numpy(q).to(gpu_device), torch.from_numpy(c).to(gpu_device)
    dt = torch.from_numpy(target).to(gpu_device)
    stream = _lib.current_stream_ptr()
    names = ("argmax", "rank", "max", "gold", "lse")

    def call(nq, nc, dim, outs, tgt=dt):
        ptrs = [outs[n].data_ptr() if n in outs else None for n in names]
        return lib.proqa_inbatch_eval_f16(dq.data_ptr(), dc.data_ptr(), tgt.data_ptr() if tgt is not None else None, nq, nc,
                                          dim, *ptrs, stream)

    for name in names:                      # every output alone
        buf = torch.full((33,), -7, dtype=torch.int32 if name in ("argmax", "rank") else torch.float32, device=gpu_device)
        assert call(33, 65, 128, {name: buf}) == 0
        assert np.array_equal(buf.cpu().numpy(), full[name]), name
    assert call(33, 65, 128, {}) == 0       # all NULL
    canary = torch.full((33,), -7, dtype=torch.int32, device=gpu_device)
    assert call(0, 65, 128, {"argmax": canary}) == 0 and call(0, 0, 128, {"argmax": canary}) == 0     # nq == 0: nothing
    torch.cuda.synchronize()
    assert (canary == -7).all()
    for dim in (64, 127, 256, 0):
        assert call(33, 65, dim, {"argmax": canary}) == -1
        assert b"dim" in lib.proqa_last_error()
    assert call(65, 33, 128, {"argmax": canary}, tgt=None) == -1            # implicit target i needs nq <= nc
    assert b"nq <= nc" in lib.proqa_last_error()
    assert call(33, 0, 128, {"argmax": canary}) == -1 and call(-1, 65, 128, {"argmax": canary}) == -1
    torch.cuda.synchronize()
    assert (canary == -7).all()
    # the Python surface raises on the same conditions
    from proqa_amd.inbatch import inbatch_eval, inbatch_accuracy_and_loss
    with pytest.raises(_lib.ProqaError):
        inbatch_eval(dc, dq)                # 65 rows against 33 columns, no target
    with pytest.raises(_lib.ProqaError):
        inbatch_eval(dq[:, :64].contiguous(), dc[:, :64].contiguous())
    with pytest.raises(ValueError, match="must be float16"):
        inbatch_eval(dq.float(), dc)           # no silent rounding, no host round trip to check
    # a target outside [0, nc): gold NaN and rank -1 for that row only
    bad = target.copy()
    bad[4], bad[9] = 65, -1
    got = run(gpu_device, q, c, bad)
    ok = np.ones(33, bool)
    ok[[4, 9]] = False
    assert (got["rank"][~ok] == -1).all() and np.isnan(got["gold"][~ok]).all()
    assert np.array_equal(got["rank"][ok], full["rank"][ok]) and np.array_equal(got["argmax"], full["argmax"])
    # one host copy of (correct, sum of lse - gold)
    n_ok, loss = inbatch_accuracy_and_loss(dq, dc, dt)
    want = oracle.inbatch_eval(q, c, target)
    assert n_ok == int((want["argmax"] == target).sum())
    assert abs(loss - float((want["lse"] - want["gold"]).sum())) <= float(lse_tolerance(q, c, want["lse"]).sum())


def test_split_calls_on_two_streams_do_not_share_partials(gpu_device):
    """The column-split path keeps its partial results in one workspace per device: calls enqueued on two streams are
    ordered by the library, so each gives what it gives alone."""
    from proqa_amd.inbatch import inbatch_eval
    cases = [integer_case(8, 20000, seed=s) for s in (1, 2)]
    dev_cases = [tuple(torch.from_numpy(x).to(gpu_device) for x in case) for case in cases]
    alone = [run(gpu_device, *case) for case in cases]
    assert not np.array_equal(alone[0]["argmax"], alone[1]["argmax"])
    streams = [torch.cuda.Stream(device=gpu_device) for _ in range(2)]
    torch.cuda.synchronize()
    outs = []
    for rep in range(6):
        k = rep % 2
        with torch.cuda.stream(streams[k]):
            outs.append((k, inbatch_eval(*dev_cases[k])))
    torch.cuda.synchronize()
    for k, out in outs:
        for key in ("argmax", "rank", "max", "gold", "lse"):
            assert np.array_equal(out[key].cpu().numpy(), alone[k][key]), (k, key)


# ---- 6: predict on the reference's planted batches -----------------------------------------------------------------------

class StubModel:
    def __init__(self, batches, dev):
        self.batches = [(torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev)) for q, c in batches]

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def __call__(self, batch):
        q, c = self.batches[batch["batch"]]
        return {"q": q, "c": c}


def test_predict_reproduces_the_reference_on_its_planted_batches(gpu_device, capsys):
    from proqa_amd import train_retriever
    with open(os.path.join(GOLDEN, "retriever_eval_golden.json")) as f:
        p = json.load(f)["predict"]
    batches = [(np.asarray(q, np.float16), np.asarray(c, np.float16)) for q, c in zip(p["q"], p["c"])]
    stats = {}
    capsys.readouterr()
    acc = train_retriever.predict(None, StubModel(batches, gpu_device), [{"batch": i} for i in range(len(batches))],
                                  gpu_device, stats=stats)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == p["first_line"] == "evaluated 17.0 examples..."
    assert isinstance(acc, float) and acc == p["acc"] and lines[1] == f"avg. Acc: {acc}" == p["second_line_reference"]
    assert stats["examples"] == p["num_total"] == 17 and stats["correct"] == 15 and stats["acc"] == acc
    # per batch: the reference's argmax
    from proqa_amd.inbatch import inbatch_eval
    for (q, c), want in zip(StubModel(batches, gpu_device).batches, p["argmax"]):
        assert inbatch_eval(q, c)["argmax"].tolist() == want
    # loss and MRR of the stats against the oracle (integer scores: exact ranks)
    o = [oracle.inbatch_eval(q, c) for q, c in batches]
    assert stats["mrr"] == pytest.approx(sum((1.0 / (x["rank"] + 1.0)).sum() for x in o) / 17, rel=1e-12)
    want_loss = sum((x["lse"] - x["gold"]).sum() for x in o) / 17
    assert abs(stats["loss"] - want_loss) <= sum(lse_tolerance(q, c, x["lse"]).sum() for (q, c), x in zip(batches, o)) / 17


# ---- 7: BertForRetriever.__call__ ------------------------------------------------------------------------------------------

def load_golden_model(dev):
    from proqa_amd.retriever import BertForRetriever
    z = np.load(os.path.join(GOLDEN, "encoder_golden.npz"))
    sd = {k[3:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w::")}
    with open(os.path.join(GOLDEN, "encoder_config.json")) as f:
        cfg = json.load(f)
    model = BertForRetriever(cfg, device=dev)
    model.load_state_dict(sd)
    return z, sd, cfg, model.eval()


def test_model_call_runs_both_towers_like_get_embed(gpu_device):
    from test_encoder_gpu import TOL_GOLDEN
    z, _, _, model = load_golden_model(gpu_device)
    ids = torch.from_numpy(z["input_ids"]).to(gpu_device)
    mask = torch.from_numpy(z["input_mask"]).to(gpu_device)
    # the question side is the first 20 columns of the same rows (right-padded like re_collate's)
    ids_q, mask_q = ids[:, :20].contiguous(), mask[:, :20].contiguous()
    out = model({"input_ids_q": ids, "input_mask_q": mask, "input_ids_c": ids, "input_mask_c": mask})
    assert set(out) == {"q", "c"}
    for key, is_q, gold in (("q", True, "embed_q"), ("c", False, "embed_c")):
        emb = model.get_embed({"input_ids": ids, "input_mask": mask}, is_q)["embed"]
        assert out[key].shape == (32, 128) and out[key].dtype == torch.float16 and out[key].is_cuda
        assert torch.equal(out[key].view(torch.int16), emb.view(torch.int16))
        assert np.abs(out[key].float().cpu().numpy() - z[gold]).max() < TOL_GOLDEN
    out2 = model({"input_ids_q": ids_q, "input_mask_q": mask_q, "input_ids_c": ids, "input_mask_c": mask})
    emb_q = model.get_embed({"input_ids": ids_q, "input_mask": mask_q}, True)["embed"]
    assert torch.equal(out2["q"].view(torch.int16), emb_q.view(torch.int16))
    assert torch.equal(out2["c"].view(torch.int16), out["c"].view(torch.int16))


# ---- 8: the command line -------------------------------------------------------------------------------------------------

def test_command_line_end_to_end(gpu_device, tmp_path, capsys, monkeypatch):
    from transformers import BertTokenizer
    from proqa_amd import datasets, train_retriever
    model_dir = tmp_path / "small-bert"
    model_dir.mkdir()
    shutil.copy(os.path.join(GOLDEN, "vocab_small.txt"), model_dir / "vocab.txt")
    z, sd, cfg, model = load_golden_model(gpu_device)
    (model_dir / "config.json").write_text(json.dumps(dict(cfg, model_type="bert")))
    torch.save({"module." + k: v for k, v in sd.items()}, tmp_path / "checkpoint_best.pt")
    gold = json.load(open(os.path.join(GOLDEN, "recall_golden.json")))
    pairs = [{"Question": qa["question"], "Paragraph": text, "Answer": qa["answer"][0]}
             for qa, (_, text) in zip(gold["qas"], gold["docs"])]
    pairs += [{"Question": f"what is {text.split()[0] if text.split() else 'it'}", "Paragraph": text}
              for _, text in gold["docs"][len(pairs):]]
    pairs += [{"Question": "", "Paragraph": "the river runs by the city " * 30},
              {"Question": "who was the first president of the united states " * 3, "Paragraph": "George Washington"},
              {"Question": "café naïve", "Paragraph": "[SEP] literal special token"}]
    pairs = pairs[:23]
    assert len(pairs) == 23
    dev_file = tmp_path / "dev.txt"
    dev_file.write_text("".join(json.dumps(p) + "\n" for p in pairs))
    stats_file = tmp_path / "stats.json"
    monkeypatch.setenv("PROQA_STATS_JSON", str(stats_file))
    capsys.readouterr()
    acc = train_retriever.main(["--do_predict", "--predict_file", str(dev_file), "--init_checkpoint",
                                str(tmp_path / "checkpoint_best.pt"), "--bert_model_name", str(model_dir),
                                "--predict_batch_size", "7", "--eval-workers", "2", "--efficient_eval",
                                "--max_seq_length", str(cfg["max_position_embeddings"])])   # the small model's 128 positions
    printed = capsys.readouterr().out.splitlines()
    stats = json.loads(stats_file.read_text())

    # the oracle on model(batch)'s embeddings, batch by batch (ReDataset + re_collate: the reference's own loader shape)
    tok = BertTokenizer.from_pretrained(str(model_dir))
    ds = datasets.ReDataset(tok, str(dev_file), 30, cfg["max_position_embeddings"])
    assert max(ds[i]["input_ids_c"].numel() for i in range(23)) == cfg["max_position_embeddings"] - 30   # one is truncated
    model.half()
    correct, loss, mrr, undecided, tol = 0, 0.0, 0.0, 0, 0.0
    for b0 in range(0, 23, 7):
        batch = datasets.re_collate([ds[i] for i in range(b0, min(b0 + 7, 23))])
        out = model({k: v.to(gpu_device) for k, v in batch.items()})
        q, c = out["q"].cpu().numpy(), out["c"].cpu().numpy()
        assert q.dtype == np.float16
        o = oracle.inbatch_eval(q, c)
        keep_argmax, keep_rank, _ = decided_rows(q, c, None)
        undecided += int((~(keep_argmax & keep_rank)).sum())
        correct += int((o["argmax"] == np.arange(len(q))).sum())
        loss += float((o["lse"] - o["gold"]).sum())
        mrr += float((1.0 / (o["rank"] + 1.0)).sum())
        tol += float(lse_tolerance(q, c, o["lse"]).sum() + np.diag(oracle.accumulation_bound(q, c)).sum())   # lse and gold
    print("undecided rows", undecided, "of 23")
    # every row is decided: the closest gold is several bounds (2.3e-5) from its neighbour on these embeddings
    assert undecided == 0
    want_acc = float(np.float32(correct) / np.float32(23))
    assert printed[-3:] == ["evaluated 23.0 examples...", f"avg. Acc: {want_acc}", str(want_acc)]
    assert acc == want_acc and stats["acc"] == want_acc and stats["correct"] == correct
    assert stats["mrr"] == pytest.approx(mrr / 23, rel=1e-12)
    assert stats["examples"] == 23 and abs(stats["loss"] - loss / 23) <= tol / 23
    assert set(stats["seconds"]) == {"load", "encode", "score"} and all(v >= 0 for v in stats["seconds"].values())
