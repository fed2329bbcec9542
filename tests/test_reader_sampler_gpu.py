"""proqa_amd.online_sampler.OnlineSampler on the MI355X against tests/golden/reader_sampler_golden.json (the reference's
OnlineSampler.load over the inputs of tests/reader_sampler_inputs.py): every yielded batch, the rows, the labels, and the
number of transfers per question."""
import json
import os

import numpy as np
import pytest

import reader_sampler_inputs as gen

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class StandInRetriever:
    """get_embed returns the generator's vector of the question (found by its token ids); records the mode it ran in"""

    def __init__(self, tokenizer, inputs, device):
        import torch
        self.by_ids = {tuple(tokenizer.encode(q["question"], max_length=gen.MAX_QUERY_LENGTH, truncation=True)): i
                       for i, q in enumerate(inputs["questions"])}
        self.vectors = torch.from_numpy(inputs["q_vectors"]).to(device).half()
        self.training = True
        self.modes = []

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    def get_embed(self, batch, is_query_embed):
        import torch
        assert is_query_embed and not torch.is_grad_enabled()
        assert batch["input_ids"].is_cuda and batch["input_mask"].all()
        self.modes.append(self.training)
        return {"embed": self.vectors[self.by_ids[tuple(batch["input_ids"].view(-1).tolist())]].view(1, -1)}


@pytest.fixture(scope="module")
def setup(gpu_device, tmp_path_factory):
    from transformers import BertTokenizer
    from proqa_amd.utils import DocDB
    tmp = str(tmp_path_factory.mktemp("reader_sampler"))
    with open(os.path.join(GOLDEN, "vocab_small.txt")) as f, open(os.path.join(tmp, "vocab.txt"), "w") as g:
        g.write(f.read())
    tokenizer = BertTokenizer.from_pretrained(tmp)
    inputs = gen.make_inputs(os.path.join(GOLDEN, "vocab_small.txt"))
    paths = gen.write_files(inputs, tmp)
    with open(os.path.join(GOLDEN, "reader_sampler_golden.json")) as f:
        golden = json.load(f)
    return tokenizer, inputs, paths, DocDB(paths["db"]), golden


def _pairs(starts, ends):
    return [sorted((s, e) for s, e in zip(a, b) if s >= 0) for a, b in zip(starts, ends)]


def test_every_batch_is_the_reference_s(setup, gpu_device):
    import torch
    from proqa_amd.online_sampler import OnlineSampler
    from proqa_amd.qa_utils import hash_question
    tokenizer, inputs, paths, db, golden = setup
    sampler = OnlineSampler(paths["raw"], tokenizer, gen.MAX_QUERY_LENGTH, gen.MAX_LENGTH, db, np.load(paths["npy"]),
                            index2paraid=paths["idx"], matched_para_path=paths["matched"])
    assert len(sampler) == 8
    retriever = StandInRetriever(tokenizer, inputs, gpu_device)
    rows16 = inputs["rows"]
    n = 0
    for q, (batch, rec) in enumerate(zip(sampler.load(retriever, k=gen.K), golden["questions"])):
        n += 1
        assert sampler.transfers == {"d2h": n, "h2d": sum(1 for r in golden["questions"][:n] if r)}
        assert bool(batch) == bool(rec), q
        if not rec:
            assert batch == {}
            continue
        ni = batch["net_input"]
        assert all(t.is_cuda for t in ni.values())
        L = len(rec["input_ids"][0])
        lens = torch.tensor(rec["seq_lens"])
        runs = torch.tensor(rec["paragraph_mask_runs"])
        ar = torch.arange(L)[None]
        assert ni["input_ids"].dtype == torch.int64 and ni["input_ids"].cpu().tolist() == rec["input_ids"]
        assert ni["segment_ids"].dtype == torch.int64 and ni["segment_ids"].cpu().tolist() == rec["segment_ids"]
        assert ni["input_mask"].dtype == torch.int64 and torch.equal(ni["input_mask"].cpu(), (ar < lens[:, None]).long())
        assert ni["paragraph_mask"].dtype == torch.bool
        assert torch.equal(ni["paragraph_mask"].cpu(), (ar >= runs[:, :1]) & (ar < runs[:, 1:]))
        assert ni["input_ids_q"].cpu().tolist() == rec["input_ids_q"] and bool(ni["input_mask_q"].all())
        assert ni["input_mask_q"].shape == ni["input_ids_q"].shape
        starts, ends = ni["start_positions"].cpu().tolist(), ni["end_positions"].cpu().tolist()
        assert np.shape(starts) == np.shape(rec["start_positions"]) == np.shape(ends)
        assert _pairs(starts, ends) == _pairs(rec["start_positions"], rec["end_positions"])
        assert all((s < 0) == (e < 0) for a, b in zip(starts, ends) for s, e in zip(a, b))
        assert all(row == sorted(row, key=lambda v: v < 0) for row in starts)        # the -1 padding follows the positions
        assert tuple(ni["para_targets"].shape) == (gen.K, 1) and ni["para_targets"].view(-1).cpu().tolist() == rec["para_targets"]
        assert batch["para_offset"] == rec["para_offset"]
        assert ni["top5000_labels"].dtype == torch.int32 and tuple(ni["top5000_labels"].shape) == (gen.K_SEARCH,)
        assert torch.nonzero(ni["top5000_labels"]).view(-1).cpu().tolist() == rec["label_positions"]
        # the rows of the recorded ids: first K and the last here, and all 5000 by the generator's own retrieval
        assert ni["para_embed"].dtype == torch.float16 and tuple(ni["para_embed"].shape) == (gen.K_SEARCH, 128)
        got = ni["para_embed"].cpu().numpy()
        np.testing.assert_array_equal(got[:gen.K], rows16[rec["first_ids"]])
        np.testing.assert_array_equal(got[-1], rows16[rec["last_id"]])
        np.testing.assert_array_equal(got, rows16[inputs["top"][q]])
        assert batch["id"] == [hash_question(inputs["questions"][q]["question"])] * gen.K
        assert batch["q"] == [inputs["questions"][q]["question"]] * gen.K
        assert batch["true_answers"] == [inputs["questions"][q]["answer"]] * gen.K
        assert all(len(t) >= m - rec["para_offset"][0] - 1 for t, m in zip(batch["wp_tokens"], rec["seq_lens"]))
    assert n == 8
    assert retriever.modes == [False] * 8 and retriever.training is True       # eval() for the pass, restored afterwards
    assert set(sampler.seconds) == {"encode", "search_collect", "host_text", "h2d"} and all(v > 0 for v in sampler.seconds.values())
    # a second pass finds every passage in the cache and yields the same
    again = [b for b in sampler.load(retriever, k=gen.K)]
    assert [bool(b) for b in again] == [bool(r) for r in golden["questions"]]
    for b, rec in zip(again, golden["questions"]):
        if rec:
            assert b["net_input"]["input_ids"].cpu().tolist() == rec["input_ids"]
            assert _pairs(b["net_input"]["start_positions"].cpu().tolist(), b["net_input"]["end_positions"].cpu().tolist()) == \
                _pairs(rec["start_positions"], rec["end_positions"])
    assert sampler.transfers == {"d2h": 16, "h2d": 14}


def test_one_copy_down_and_one_copy_up_per_question_with_the_real_tower(setup, gpu_device, monkeypatch):
    """The transfers of a pass, MEASURED, with the model's own TrainableRetriever as the retriever (its tower pass would
    read its mask back without the host-lengths path).  A profile of the second pass (caches and workspaces warm) counts the
    runtime's memcpy records: `Memcpy DtoH` must be one per question -- the record -- and there must be no `Memcpy HtoD`
    (a pageable upload) at all.  The profiler files a copy out of PINNED host memory under DtoD (the buffer is
    device-addressable), so the batch's upload is counted where it is issued: every Tensor.copy_ / .to / .cuda whose
    source is a pinned host tensor and whose destination is the device -- one per non-empty batch."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    import train_oracle
    from proqa_amd.online_sampler import OnlineSampler
    from proqa_amd.reader import random_state_dict
    from proqa_amd.trainable_reader import TrainableReader
    tokenizer, inputs, paths, db, _ = setup
    cfg = dict(train_oracle.SMALL_CONFIG, vocab_size=512)
    model = TrainableReader(cfg, gpu_device)
    model.load_state_dict(random_state_dict(cfg, seed=2, std=0.03))
    model.train()
    sampler = OnlineSampler(paths["raw"], tokenizer, gen.MAX_QUERY_LENGTH, gen.MAX_LENGTH, db, np.load(paths["npy"]),
                            index2paraid=paths["idx"], matched_para_path=paths["matched"])
    warm = [bool(b) for b in sampler.load(model.retriever, k=gen.K)]
    torch.cuda.synchronize()
    pinned_up = []
    real_copy, real_to, real_cuda = torch.Tensor.copy_, torch.Tensor.to, torch.Tensor.cuda

    def copy_(self, src, *a, **k):
        if self.is_cuda and isinstance(src, torch.Tensor) and not src.is_cuda and src.is_pinned():
            pinned_up.append(src.numel())
        return real_copy(self, src, *a, **k)

    def to(self, *a, **k):
        out = real_to(self, *a, **k)
        if not self.is_cuda and out.is_cuda and self.is_pinned():
            pinned_up.append(self.numel())
        return out

    def cuda(self, *a, **k):
        if not self.is_cuda and self.is_pinned():
            pinned_up.append(self.numel())
        return real_cuda(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "copy_", copy_)
    monkeypatch.setattr(torch.Tensor, "to", to)
    monkeypatch.setattr(torch.Tensor, "cuda", cuda)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        batches = [bool(b) for b in sampler.load(model.retriever, k=gen.K)]
        torch.cuda.synchronize()
    monkeypatch.undo()
    names = [e.name for e in prof.events() if e.name.startswith("Memcpy")]
    d2h = sum(1 for n in names if n.startswith("Memcpy DtoH"))
    h2d = sum(1 for n in names if n.startswith("Memcpy HtoD"))
    print("memcpy records of 8 questions:", {n: names.count(n) for n in set(names)}, "pinned uploads:", pinned_up)
    assert batches == warm and len(batches) == 8 and 0 < sum(batches)
    assert any(n.startswith("Memcpy") for n in names)          # the profile did record copies
    assert d2h == 8                                            # one per question: the record
    assert h2d == 0 and len(pinned_up) == sum(batches)         # one per non-empty batch, out of the pinned buffer
    assert model.retriever.training


def test_an_index_smaller_than_the_search_yields_its_rows(setup, gpu_device):
    import torch
    from proqa_amd.index import IndexFlatIP
    from proqa_amd.online_sampler import OnlineSampler
    tokenizer, inputs, paths, db, _ = setup
    index = IndexFlatIP(128)
    index.add(inputs["rows"][:600])
    sampler = OnlineSampler(paths["raw"], tokenizer, gen.MAX_QUERY_LENGTH, gen.MAX_LENGTH, db, index,
                            index2paraid=[gen.para_id(r) for r in range(600)], matched_para_path=paths["matched"])
    retriever = StandInRetriever(tokenizer, inputs, gpu_device)
    scores = inputs["q_vectors"].astype(np.float64) @ inputs["rows"][:600].astype(np.float64).T
    seen = 0
    for q, batch in enumerate(sampler.load(retriever, k=gen.K)):
        if not batch:
            continue
        seen += 1
        ni = batch["net_input"]
        assert tuple(ni["para_embed"].shape) == (600, 128) and tuple(ni["top5000_labels"].shape) == (600,)
        order = np.argsort(-scores[q], kind="stable")
        np.testing.assert_array_equal(ni["para_embed"].cpu().numpy(), inputs["rows"][order])
        gold = {r for r in range(600) if gen.para_id(r) in inputs["matched"][q]["matched_paras"]}
        assert torch.nonzero(ni["top5000_labels"]).view(-1).cpu().tolist() == [i for i, r in enumerate(order) if r in gold]
        assert ni["input_ids"].shape[0] == gen.K
    assert seen > 0


def test_refusals(setup, gpu_device):
    from proqa_amd.online_sampler import OnlineSampler
    tokenizer, inputs, paths, db, _ = setup
    rows = np.load(paths["npy"])[:64]
    common = dict(index2paraid=paths["idx"])
    with pytest.raises(ValueError, match="matched_para_path"):
        OnlineSampler(paths["raw"], tokenizer, 12, 48, db, rows, matched_para_path="", **common)
    with pytest.raises(ValueError, match="cased"):
        OnlineSampler(paths["raw"], tokenizer, 12, 48, db, rows, matched_para_path=paths["matched"], cased=True, **common)
    short = os.path.join(os.path.dirname(paths["matched"]), "matched_short.txt")
    with open(paths["matched"]) as f, open(short, "w") as g:
        g.writelines(f.readlines()[:5])
    with pytest.raises(ValueError, match=inputs["questions"][5]["question"]):
        OnlineSampler(paths["raw"], tokenizer, 12, 48, db, rows, matched_para_path=short, **common)
