"""OnlineSampler.retrieve_many / load(lookahead=...) and train_reader.py --sampler-lookahead on the MI355X.

The sampler is compared with itself, question by question, under a stand-in retriever whose get_embed is a ROW-WISE
function of the token ids: the sum, over the row's tokens, of rows of a table with entries m/8 (at most 12 tokens: every
sum is exact in float32 and in the fp16 it is cast to), so a batch and its rows encoded alone agree to the bit and any
difference is the sampler's.  Through the real tower only the plumbing is checked (the embeddings searched are the bits of
one direct get_embed call on the same padded ids): a tower pass over several questions need not give the bits of the passes
over one, and no test here compares the two.

train_reader.py: the tiny model and files of tests/test_train_reader_gpu.py, G = 4 (update slots at the batch steps 3, 7,
11), so --sampler-lookahead 4 retrieves [1, 2, 3], [4, 5, 6, 7], [8] in the first epoch and [9, 10, 11] in the second, where
the runs stop after their third update.
"""
import json
import os

import numpy as np
import pytest

import reader_sampler_inputs as gen
from test_train_reader_gpu import _argv, setup      # noqa: F401  (the module-scoped fixture, built again here)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = 4
FLAGS = ("--deterministic", "--learning_rate", "1e-3", "--gradient_accumulation_steps", str(G), "--digest-every", "1",
         "--save-state", "--save_checkpoints_steps", "1")
AHEAD = ("--sampler-lookahead", "4", "--questions-per-pass", "4")


class TableRetriever:
    """get_embed: the rows of an integer table summed over each row's tokens (the padding's row is zero), as fp16"""

    def __init__(self, device, vocab=512, seed=2207):
        import torch
        table = np.random.default_rng(seed).integers(-8, 9, (vocab, 128)) / 8.0
        table[0] = 0
        self.table = torch.from_numpy(table.astype(np.float32)).to(device)
        self.training = True
        self.modes, self.batch_sizes = [], []

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    def get_embed(self, batch, is_query_embed):
        import torch
        assert is_query_embed and not torch.is_grad_enabled()
        ids, mask = batch["input_ids"], batch["input_mask"]
        assert ids.is_cuda and ids.dim() == 2 and mask.shape == ids.shape and mask.dtype == torch.bool
        assert bool(((ids != 0) == mask).all())           # right-padded with 0, the mask a prefix of ones
        self.modes.append(self.training)
        self.batch_sizes.append(ids.shape[0])
        return {"embed": (self.table[ids] * mask[..., None]).sum(dim=1).half()}


@pytest.fixture(scope="module")
def corpus(gpu_device, tmp_path_factory):
    from transformers import BertTokenizer
    from proqa_amd.utils import DocDB
    tmp = str(tmp_path_factory.mktemp("sampler_lookahead"))
    with open(os.path.join(GOLDEN, "vocab_small.txt")) as f, open(os.path.join(tmp, "vocab.txt"), "w") as g:
        g.write(f.read())
    tokenizer = BertTokenizer.from_pretrained(tmp)
    inputs = gen.make_inputs(os.path.join(GOLDEN, "vocab_small.txt"))
    paths = gen.write_files(inputs, tmp)
    return tokenizer, inputs, paths, DocDB(paths["db"])


def _sampler(corpus):
    from proqa_amd.online_sampler import OnlineSampler
    tokenizer, _, paths, db = corpus
    return OnlineSampler(paths["raw"], tokenizer, gen.MAX_QUERY_LENGTH, gen.MAX_LENGTH, db, np.load(paths["npy"]),
                         index2paraid=paths["idx"], matched_para_path=paths["matched"])


@pytest.fixture(scope="module")
def one_by_one(corpus, gpu_device):
    """(the sampler, retrieve() of every question, load() of the epoch) under the table retriever: computed once"""
    sampler = _sampler(corpus)
    retriever = TableRetriever(gpu_device)
    singles = [sampler.retrieve(retriever, qa["question"], gen.K) for qa in sampler.qa_data]
    batches = list(sampler.load(retriever, k=gen.K))
    assert retriever.batch_sizes == [1] * 16 and retriever.modes == [False] * 16 and retriever.training
    assert sum(1 for b in batches if b == {}) >= 1 and sum(1 for b in batches if b) >= 4
    return sampler, singles, batches


def _same_retrieval(got, want):
    import torch
    assert got[0] == want[0] and got[3:] == want[3:]              # q_ids; n_live, n_gold, head rows
    for a, b in zip(got[1:3], want[1:3]):                         # rows and labels, bit for bit
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.view(torch.uint8))


def _same_batch(got, want):
    import torch
    assert bool(got) == bool(want)
    if not want:
        assert got == {}
        return
    assert set(got) == set(want) and set(got["net_input"]) == set(want["net_input"])
    for key in want:
        if key != "net_input":
            assert got[key] == want[key], key
    for key, t in want["net_input"].items():
        g = got["net_input"][key]
        assert g.dtype == t.dtype and g.shape == t.shape and torch.equal(g, t), key


def test_the_stand_in_is_row_wise(corpus, one_by_one, gpu_device):
    import torch
    sampler, _, _ = one_by_one
    retriever = TableRetriever(gpu_device)
    ids, mask = sampler._q_ids_dev, sampler._q_mask_dev
    assert len({len(t) for t in sampler._q_ids}) > 2              # questions of several lengths: the batch is padded
    with torch.no_grad():
        batch = retriever.get_embed({"input_ids": ids, "input_mask": mask}, True)["embed"]
        for i, t in enumerate(sampler._q_ids):
            alone = retriever.get_embed({"input_ids": ids[i:i + 1, :len(t)], "input_mask": mask[i:i + 1, :len(t)]}, True)["embed"]
            assert torch.equal(alone[0], batch[i])
    assert len({tuple(r) for r in batch.cpu().tolist()}) == len(sampler._q_ids)


@pytest.mark.parametrize("n", [1, 4, 8])
def test_retrieve_many_is_retrieve_question_by_question(one_by_one, gpu_device, n):
    sampler, singles, _ = one_by_one
    retriever = TableRetriever(gpu_device)
    questions = [qa["question"] for qa in sampler.qa_data]
    before, groups = dict(sampler.transfers), sampler.groups
    for at in range(0, len(questions), n):
        got = sampler.retrieve_many(retriever, questions[at:at + n], gen.K)
        assert len(got) == n
        for g, want in zip(got, singles[at:at + n]):
            _same_retrieval(g, want)
    calls = len(questions) // n
    assert retriever.batch_sizes == [n] * calls and retriever.modes == [False] * calls and retriever.training
    assert sampler.transfers == {"d2h": before["d2h"] + calls, "h2d": before["h2d"]} and sampler.groups == groups + calls
    assert sum(w[4] for w in singles) > 0 and any(w[3] == gen.K_SEARCH for w in singles)


def test_a_question_twice_in_a_group(one_by_one, gpu_device):
    sampler, singles, _ = one_by_one
    questions = [qa["question"] for qa in sampler.qa_data]
    got = sampler.retrieve_many(TableRetriever(gpu_device), [questions[2], questions[7], questions[2]], gen.K)
    for g, want in zip(got, (singles[2], singles[7], singles[2])):
        _same_retrieval(g, want)
    assert sampler.retrieve_many(TableRetriever(gpu_device), [], gen.K) == []
    with pytest.raises(ValueError, match="not one of the sampler's training questions"):
        sampler.retrieve_many(TableRetriever(gpu_device), [questions[0], "a question nobody asked"], gen.K)


@pytest.mark.parametrize("n", [1, 3, 8, 100])
def test_load_with_lookahead_yields_load_s_sequence(corpus, one_by_one, gpu_device, n):
    """groups of 1, of 3 (3 + 3 + 2), the whole epoch, and a lookahead past the epoch's end"""
    _, _, batches = one_by_one
    sampler = _sampler(corpus)
    retriever = TableRetriever(gpu_device)
    asked = []

    def lookahead():
        asked.append(sampler.questions_seen)
        return n
    got = list(sampler.load(retriever, k=gen.K, lookahead=lookahead))
    assert len(got) == len(batches) == 8
    for g, want in zip(got, batches):
        _same_batch(g, want)
    n_groups = -(-8 // n)
    assert asked == list(range(0, 8, n))              # asked when everything retrieved has been yielded, and only then
    assert retriever.batch_sizes == [min(n, 8 - at) for at in asked]
    assert sampler.transfers["d2h"] == n_groups == sampler.groups
    assert sampler.transfers["h2d"] == sum(1 for b in batches if b) and sampler.questions_seen == 8
    # a resumed epoch: the groups start at `start`
    tail = list(sampler.load(retriever, k=gen.K, start=5, lookahead=lambda: n))
    assert len(tail) == 3
    for g, want in zip(tail, batches[5:]):
        _same_batch(g, want)
    assert sampler.transfers["d2h"] == n_groups + -(-3 // n)


def test_a_consumer_that_stops_early(corpus, gpu_device):
    sampler = _sampler(corpus)
    it = sampler.load(TableRetriever(gpu_device), k=gen.K, lookahead=lambda: 3)
    next(it), next(it)
    it.close()
    assert sampler.questions_seen == 2 and sampler.transfers["d2h"] == 1 and sampler.groups == 1
    with pytest.raises(ValueError, match="at least 1"):
        next(sampler.load(TableRetriever(gpu_device), k=gen.K, lookahead=lambda: 0))


def test_the_real_tower_sees_one_padded_batch(corpus, gpu_device, monkeypatch):
    """plumbing only: one get_embed call over the right-padded ids with the host lengths, in eval() under no_grad; the
    embeddings handed to the search are that call's bits, which are the bits of a direct call; train() afterwards"""
    import torch
    import train_oracle
    from proqa_amd.qa_utils import hash_question
    from proqa_amd.reader import random_state_dict
    from proqa_amd.trainable_reader import TrainableReader
    cfg = dict(train_oracle.SMALL_CONFIG, vocab_size=512)
    model = TrainableReader(cfg, gpu_device)
    model.load_state_dict(random_state_dict(cfg, seed=2, std=0.03))
    model.train()
    retriever = model.retriever
    sampler = _sampler(corpus)
    questions = [qa["question"] for qa in sampler.qa_data][:5]
    real_get_embed, real_search = retriever.get_embed, sampler.index.search_device
    calls, searched = [], []

    def get_embed(batch, is_query_embed, check_mask=True, seq_lens_host=None):
        calls.append((batch["input_ids"].clone(), batch["input_mask"].clone(), is_query_embed, check_mask, list(seq_lens_host),
                      retriever.training, torch.is_grad_enabled()))
        return real_get_embed(batch, is_query_embed, check_mask=check_mask, seq_lens_host=seq_lens_host)

    def search_device(xq, k, *a, **kw):
        searched.append((xq.clone(), k))
        return real_search(xq, k, *a, **kw)

    monkeypatch.setattr(retriever, "get_embed", get_embed)
    monkeypatch.setattr(sampler.index, "search_device", search_device)
    before = dict(sampler.transfers)
    out = sampler.retrieve_many(retriever, questions, gen.K)
    monkeypatch.undo()
    assert retriever.training and len(out) == 5 and len(calls) == 1 and len(searched) == 1
    ids, mask, is_query, check_mask, lens, training, grad = calls[0]
    q_ids = [sampler._q_ids[sampler._gold_slot[hash_question(q)]] for q in questions]
    assert lens == [len(t) for t in q_ids] and len(set(lens)) > 1 and tuple(ids.shape) == (5, max(lens))
    assert ids.cpu().tolist() == [list(t) + [0] * (max(lens) - len(t)) for t in q_ids]
    assert torch.equal(mask.cpu(), torch.arange(max(lens))[None] < torch.tensor(lens)[:, None])
    assert is_query is True and check_mask is False and training is False and grad is False
    assert searched[0][1] == 5000 and tuple(searched[0][0].shape) == (5, 128) and searched[0][0].dtype == torch.float16
    retriever.eval()
    with torch.no_grad():
        direct = retriever.get_embed({"input_ids": ids, "input_mask": mask}, True, check_mask=False, seq_lens_host=lens)["embed"]
    retriever.train()
    assert torch.equal(searched[0][0].view(torch.int16), direct.reshape(5, 128).view(torch.int16))
    assert sampler.transfers == {"d2h": before["d2h"] + 1, "h2d": before["h2d"]}
    assert [o[0] for o in out] == q_ids and all(o[3] == gen.K_SEARCH for o in out)


# ---- train_reader.py --sampler-lookahead -----------------------------------------------------------------------------------
def _run(setup, out, *flags, init=True):        # noqa: F811
    from proqa_amd import train_reader
    argv = _argv(setup, out, *FLAGS, *flags)
    if not init:
        at = argv.index("--init_checkpoint")
        del argv[at:at + 2]
    stats_file = setup["root"] / f"stats-{out}.json"
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("PROQA_STATS_JSON", str(stats_file))
        train_reader.main(argv)
    finally:
        mp.undo()
    return json.loads(stats_file.read_text())


@pytest.fixture(scope="module")
def straight(gpu_device, setup):        # noqa: F811
    return _run(setup, "ahead-a", *AHEAD, "--stop-after-updates", "3")


def test_two_runs_agree_and_the_groups_are_the_schedule_s(gpu_device, setup, straight):        # noqa: F811
    from proqa_amd.train_reader import retrieval_groups
    again = _run(setup, "ahead-b", *AHEAD, "--stop-after-updates", "3")
    assert len(straight["state_digests"]) == 3 and len({d["params"] for d in straight["state_digests"]}) == 3
    for key in ("state_digests", "losses", "update_steps", "failed_steps", "batch_steps", "sampler_groups"):
        assert again[key] == straight[key], key
    assert straight["batch_steps"] == 11 and straight["update_steps"] == [3, 7, 11] and straight["global_step"] == 3
    first_epoch = retrieval_groups(8, G, 4)
    second = [g for g in retrieval_groups(8, G, 4, first=9) if g[0] <= 11]
    assert first_epoch == [[1, 2, 3], [4, 5, 6, 7], [8]] and second == [[9, 10, 11]]
    assert straight["sampler_lookahead"] == 4 and straight["sampler_groups"] == len(first_epoch) + len(second) == 4
    assert straight["sampler_transfers"]["d2h"] == 4
    log = open(os.path.join(straight["output_dir"], "log.txt")).read()
    assert log.count("--sampler-lookahead 4") == 1 and "every group holds one question" not in log


def test_resume_forms_the_groups_of_the_uninterrupted_run(gpu_device, setup, straight):        # noqa: F811
    half = _run(setup, "ahead-halves", *AHEAD, "--stop-after-updates", "1")
    assert half["global_step"] == 1 and half["batch_steps"] == 3 and half["sampler_groups"] == 1
    assert half["state_digests"] == straight["state_digests"][:1]
    resumed = _run(setup, "ahead-halves", *AHEAD, "--stop-after-updates", "3", "--resume", half["output_dir"], init=False)
    for key in ("global_step", "batch_steps", "update_steps", "failed_steps", "losses", "state_digests", "loss_scale", "passes",
                "sampler_lookahead", "sampler_groups"):
        assert resumed[key] == straight[key], key
    # another --sampler-lookahead is another run
    with pytest.raises(SystemExit, match="'sampler_lookahead' is 2 now, was 4"):
        _run(setup, "ahead-halves", "--sampler-lookahead", "2", "--questions-per-pass", "4", "--stop-after-updates", "3", "--resume",
             half["output_dir"], init=False)
    with pytest.raises(SystemExit, match="'sampler_lookahead' is 1 now, was 4"):
        _run(setup, "ahead-halves", "--questions-per-pass", "4", "--stop-after-updates", "3", "--resume", half["output_dir"],
             init=False)


def test_one_question_windows_are_the_run_without_the_flag(gpu_device, setup):        # noqa: F811
    """G = 1: every question sits in an update slot, every group holds one question, and a group of one is retrieve()"""
    g1 = ("--gradient_accumulation_steps", "1", "--stop-after-updates", "3")
    plain = _run(setup, "ahead-g1-plain", *g1)
    ahead = _run(setup, "ahead-g1", "--sampler-lookahead", "4", *g1)
    assert "sampler_lookahead" not in plain and "sampler_groups" not in plain
    assert ahead["sampler_lookahead"] == 4 and ahead["sampler_groups"] == ahead["batch_steps"] == plain["batch_steps"]
    for key in ("state_digests", "losses", "update_steps", "failed_steps"):
        assert ahead[key] == plain[key], key
    assert len(plain["state_digests"]) == 3
    log = open(os.path.join(ahead["output_dir"], "log.txt")).read()
    assert log.count("every group holds one question") == 1
