"""Generate tests/golden/retriever_eval_golden.json by running the REFERENCE's own code on the CPU.

Run in the build container only (needs /root/reference, like make_golden.py):

    python tests/golden/make_retriever_eval_golden.py

R1 "dataset"  reference ReDataset + re_collate (retrieval/datasets.py:153-240) over 20 (Question, Paragraph, Answer) records
              with vocab_small.txt: the four collated tensors and filter_sample of every record, for max_query_length 6 /
              max_length 22 (every long side truncated) and 30 / 512.
R2 "predict"  reference predict (retrieval/train_retriever.py:293-333) over a stub model that returns planted
              integer-valued q / c per batch (values in [-4, 4]: every product and sum is exact in fp16 inputs / fp32
              accumulation / float64 alike).  Three batches of 7, 7 and 3 pairs; batch 0 holds two identical paragraphs,
              so one question's gold ties with a LOWER column (argmax picks the other: wrong) and one with a HIGHER column
              (argmax picks the gold: right); batch 1 has one question planted on another paragraph.
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/retrieval"

LONG = ("the river runs by the city and the university of the united states was the first school in the world "
        "war film music album band team season game")
RECORDS = [
    ("capital of france?", "Paris is the capital and most populous city of France.", "Paris"),
    ("", "an empty question still gets its two special tokens", "tokens"),
    ("who was the first president of the united states?", LONG, "george washington"),
    ("what is the river", LONG + " " + LONG, "The River"),            # answer inside the question: filtered
    ("new york state", "new york", "york"),
    ("a", "", "a"),
    ("born in 1984, he was king", "He was born in 1984.", "1984"),
    ("The band's first album was music for a film!", LONG, "album"),
    ("x y z 0 1 2 3 4 5 6 7 8 9", "0 1 2 3 4 5 6 7 8 9 " * 3, "zebra"),
    ("unknownword anotherone", "unknownword " * 25, "nothing"),
    ("Team season game (school)", LONG.upper(), "An Answer"),
    ("When, where? who - what", "when where who what " * 6, "whom"),
    ("QUEEN of the world war", "the queen", "Queen"),
    ("states' united", LONG, "states"),
    ("i j k l m n o p q r s t u v w", "i j k l m n o p q r s t u v w x y z", "w"),
    ("of and in to was is", "of and in to was is for as on with by he at from his it an are which paris", "the"),
    ("h e l l o", "h e l l o w o r l d", "hello"),
    ("Capital  of   the\tworld\nwar", "Capital  of   the\tworld\nwar and more", "peace"),
    ("which city", "paris france capital city river " * 5, "paris"),
    ("film music", "the " * 40, "a"),
]


def ref_import(name):
    sys.path.insert(0, REF)
    try:
        return __import__(name)
    finally:
        sys.path.remove(REF)


def r1_dataset():
    datasets = ref_import("datasets")
    from transformers import BertTokenizer
    out = {"records": [{"Question": q, "Paragraph": p, "Answer": a} for q, p, a in RECORDS], "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(HERE, "vocab_small.txt")) as src, open(os.path.join(tmp, "vocab.txt"), "w") as dst:
            dst.write(src.read())
        tok = BertTokenizer.from_pretrained(tmp)
        path = os.path.join(tmp, "dev.txt")
        with open(path, "w") as f:
            for r in out["records"]:
                f.write(json.dumps(r) + "\n")
        for max_q, max_len in [(6, 22), (30, 512)]:
            with contextlib.redirect_stdout(io.StringIO()):
                ds = datasets.ReDataset(tok, path, max_q, max_len)
            samples = [ds[i] for i in range(len(ds))]
            batch = datasets.re_collate(samples)
            case = {"max_query_length": max_q, "max_length": max_len,
                    "item_lengths_q": [int(s["input_ids_q"].numel()) for s in samples],
                    "item_lengths_c": [int(s["input_ids_c"].numel()) for s in samples],
                    "group_indexs": ds.group_indexs}
            for k, v in batch.items():
                case[k] = v.int().tolist()
            out["cases"].append(case)
        out["filter_sample"] = [bool(ds.filter_sample(r)) for r in out["records"]]
        with contextlib.redirect_stdout(io.StringIO()):
            out["filtered_len"] = len(datasets.ReDataset(tok, path, 6, 22, filter=True))
    assert datasets.re_collate([]) == {}
    assert max(out["cases"][0]["item_lengths_q"]) == 6 and min(out["cases"][0]["item_lengths_q"]) == 2
    assert max(out["cases"][0]["item_lengths_c"]) == 16
    assert 0 < sum(out["filter_sample"]) < len(RECORDS)
    return out


def planted_batches():
    rng = np.random.default_rng(11)
    batches = []
    for b, n in enumerate((7, 7, 3)):
        c = rng.integers(-4, 5, (n, 128)).astype(np.float32)
        if b == 0:
            c[5] = c[2]                 # rows 2 and 5: one paragraph twice
        q = c.copy()                    # s_ii = |c_i|^2: the gold wins unless planted otherwise
        if b == 1:
            q[1] = c[4]                 # question 1 is about paragraph 4
        batches.append((q, c))
    return batches


def r2_predict():
    # what the module imports at its top but predict never touches
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    ref_import("retriever")                          # (transformers' lazy module settles into sys.modules here)
    if not hasattr(sys.modules["transformers"], "AdamW"):   # gone from recent transformers; only training uses it
        sys.modules["transformers"].AdamW = torch.optim.AdamW
    tr = ref_import("train_retriever")
    tr.move_to_cuda = lambda batch: batch          # the CPU path: argmax keeps the lowest index of equal scores
    tr.tqdm = lambda it: it
    batches = planted_batches()

    class Stub:
        def __init__(self):
            self.calls = 0

        def eval(self):
            return self

        def train(self):
            return self

        def __call__(self, batch):
            q, c = batches[batch["batch"]]
            return {"q": torch.from_numpy(q), "c": torch.from_numpy(c)}

    argmaxes = []
    mm = torch.mm

    def recording_mm(a, b):
        p = mm(a, b)
        argmaxes.append(p.argmax(-1).tolist())
        return p

    buf = io.StringIO()
    torch.mm = recording_mm
    try:
        with contextlib.redirect_stdout(buf):
            acc = tr.predict(None, Stub(), [{"batch": i} for i in range(len(batches))], torch.device("cpu"))
    finally:
        torch.mm = mm
    lines = buf.getvalue().splitlines()
    acc = float(acc)
    assert 0.0 < acc < 1.0
    assert argmaxes[0][5] == 2 and argmaxes[0][2] == 2 and argmaxes[1][1] == 4
    return {"q": [q.astype(int).tolist() for q, _ in batches], "c": [c.astype(int).tolist() for _, c in batches],
            "argmax": argmaxes, "num_total": float(sum(len(q) for q, _ in batches)), "acc": acc,
            "first_line": lines[0], "second_line_reference": lines[1]}


if __name__ == "__main__":
    out = {"dataset": r1_dataset(), "predict": r2_predict()}
    with open(os.path.join(HERE, "retriever_eval_golden.json"), "w") as f:
        json.dump(out, f)
    print("R1", len(out["dataset"]["cases"]), "cases; filter", out["dataset"]["filter_sample"])
    print("R2", out["predict"]["first_line"], "|", out["predict"]["second_line_reference"], "| acc", out["predict"]["acc"])
