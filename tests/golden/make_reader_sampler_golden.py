"""Generate tests/golden/reader_sampler_golden.json by running the REFERENCE's own OnlineSampler.load on CPU.

Run in the build container only (needs the reference checkout; nothing here travels to the GPU box except the JSON it
writes):

    python tests/golden/make_reader_sampler_golden.py [path of the reference's qa/ directory]

Inputs: tests/reader_sampler_inputs.py (seeded; shared with the tests).  As in the other recipes, modules the reference
imports but this container lacks are stubbed in sys.modules (tensorflow, apex, torch.utils.tensorboard).  `faiss` is a stub
whose IndexIVFFlat.search is oracle.search_oracle.topk_ip -- the exact inner-product top k, a stable argsort with ties to
the ascending row: the search this project runs in the sampler's place.  torch.Tensor.cuda is the identity
and the retriever is a stub that returns the seeded vector of the question.  The tokenizer is transformers' BertTokenizer
over vocab_small.txt behind a proxy whose encode() truncates to max_length (the reference relies on the implicit
truncation of the transformers release it was written for).

Recorded, as integers only, per question: {} or input_ids, segment_ids, the paragraph_mask runs, start / end (the spans of
a passage sorted, so that the file does not depend on the run's hash seed),
para_targets, para_offset, the positions of the ones in top5000_labels, the first K and the last of the 5000 ids.
"""
import importlib.machinery
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/qa"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import search_oracle  # noqa: E402
import reader_sampler_inputs as gen  # noqa: E402


def stub_modules():
    for name in ("tensorflow", "apex", "torch.utils.tensorboard"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            m.SummaryWriter = object
            sys.modules[name] = m

    class _Index:
        def __init__(self, *a):
            self.xb = None
            self.nprobe = 1

        def train(self, x):
            pass

        def add(self, x):
            self.xb = np.asarray(x)

        def search(self, xq, k):
            return search_oracle.topk_ip(np.asarray(xq), self.xb, k)

    faiss = types.ModuleType("faiss")
    faiss.__spec__ = importlib.machinery.ModuleSpec("faiss", None)
    faiss.IndexFlatIP = _Index
    faiss.IndexIVFFlat = _Index
    sys.modules["faiss"] = faiss
    sys.path.insert(0, REF)
    torch.Tensor.cuda = lambda self, *a, **k: self


class TruncatingTokenizer:
    """BertTokenizer whose encode(text, max_length=n) truncates, as the reference expects"""

    def __init__(self, tok):
        self._tok = tok
        self.vocab = tok.vocab

    def encode(self, text, max_length=None):
        return self._tok.encode(text, max_length=max_length, truncation=True)

    def __getattr__(self, name):
        return getattr(self._tok, name)


class StubRetriever:
    """bert_q returns the question's position in the data as its 'pooled output'; proj_q turns it into the seeded vector"""

    def __init__(self, tok, questions, vectors):
        self.by_ids = {tuple(tok.encode(q["question"], max_length=gen.MAX_QUERY_LENGTH)): i for i, q in enumerate(questions)}
        assert len(self.by_ids) == len(questions)
        self.vectors = torch.from_numpy(vectors)

    def bert_q(self, q_ids, q_masks):
        return None, torch.tensor([self.by_ids[tuple(q_ids.view(-1).tolist())]])

    def proj_q(self, cls):
        return self.vectors[cls]


def sorted_spans(starts, ends):
    """the (start, end) pairs of every passage in ascending order, the -1 padding last: the reference appends them in the
    order of a `set` of strings, which changes with the hash seed of the run"""
    out_s, out_e = [], []
    for a, b in zip(starts, ends):
        pairs = sorted((s, e) for s, e in zip(a, b) if s >= 0)
        pad = len(a) - len(pairs)
        out_s.append([s for s, _ in pairs] + [-1] * pad)
        out_e.append([e for _, e in pairs] + [-1] * pad)
    return out_s, out_e


def runs_of(mask_row):
    on = [i for i, v in enumerate(mask_row) if v]
    assert on == list(range(on[0], on[-1] + 1)) if on else True
    return [on[0], on[-1] + 1] if on else [0, 0]


def main():
    stub_modules()
    from transformers import BertTokenizer
    from online_sampler import OnlineSampler
    from utils import DocDB
    vocab_path = os.path.join(HERE, "vocab_small.txt")
    inputs = gen.make_inputs(vocab_path)
    with tempfile.TemporaryDirectory() as tmp:
        with open(vocab_path) as f, open(os.path.join(tmp, "vocab.txt"), "w") as g:
            g.write(f.read())
        tok = TruncatingTokenizer(BertTokenizer.from_pretrained(tmp))
        paths = gen.write_files(inputs, tmp)
        sampler = OnlineSampler(paths["raw"], tok, gen.MAX_QUERY_LENGTH, gen.MAX_LENGTH, DocDB(paths["db"]),
                                inputs["rows"].astype(np.float32), index2paraid=paths["idx"], matched_para_path=paths["matched"])
        retriever = StubRetriever(tok, inputs["questions"], inputs["q_vectors"])
        records, searched = [], []
        search = sampler.index.search

        def recording_search(xq, k):
            D, I = search(xq, k)
            searched.append(I.reshape(-1))
            return D, I
        sampler.index.search = recording_search
        for batch in sampler.load(retriever, k=gen.K):
            I = searched[-1]
            np.testing.assert_array_equal(I, inputs["top"][len(records)])
            if not batch:
                records.append({})
                continue
            ni = batch["net_input"]
            np.testing.assert_array_equal(ni["para_embed"].numpy(), inputs["rows"].astype(np.float32)[I])
            assert (ni["input_mask"] == (torch.arange(ni["input_ids"].shape[1])[None] <
                                        ni["input_mask"].sum(1, keepdim=True))).all()
            starts, ends = sorted_spans(ni["start_positions"].tolist(), ni["end_positions"].tolist())
            records.append({
                "input_ids": ni["input_ids"].tolist(), "segment_ids": ni["segment_ids"].tolist(),
                "seq_lens": ni["input_mask"].sum(1).tolist(),
                "paragraph_mask_runs": [runs_of(r) for r in ni["paragraph_mask"].tolist()],
                "start_positions": starts, "end_positions": ends,
                "para_targets": ni["para_targets"].view(-1).tolist(), "para_offset": batch["para_offset"],
                "input_ids_q": ni["input_ids_q"].tolist(),
                "label_positions": torch.nonzero(ni["top5000_labels"]).view(-1).tolist(),
                "first_ids": I[:gen.K].tolist(), "last_id": int(I[-1]), "n_ids": int(len(I))})

    # the cases the fixture must contain
    assert records[0] == {}, "a question that yields {}"
    assert any(r and not r["label_positions"] and sum(r["para_targets"]) > 0 for r in records), "no gold row, a covered passage"
    assert any(r and r["label_positions"] and sum(r["para_targets"]) == 0 for r in records), "gold rows, no covered passage"
    r3 = records[3]
    long_row = inputs["passages"][int(inputs["top"][3, 0])]
    assert "river album" in long_row and r3["para_targets"][0] == 0 and r3["seq_lens"][0] == gen.MAX_LENGTH, \
        "a passage cut by max_length whose answer lies past the cut"
    assert any(r and any(sum(1 for s in row if s >= 0) >= 2 for row in r["start_positions"]) for r in records), "two spans"
    assert any(r and any(-1 in row and max(row) >= 0 for row in r["start_positions"]) for r in records), "-1 beside positions"
    out = {"k": gen.K, "max_length": gen.MAX_LENGTH, "max_query_length": gen.MAX_QUERY_LENGTH, "questions": records}
    with open(os.path.join(HERE, "reader_sampler_golden.json"), "w") as f:
        json.dump(out, f)
    print(f"wrote reader_sampler_golden.json: {sum(1 for r in records if r)} batches, {sum(1 for r in records if not r)} empty")


if __name__ == "__main__":
    main()
