"""Generate tests/golden/reader_golden.json by running the REFERENCE's own reader code on CPU.

Run in the build container only (needs the reference checkout; nothing here travels to the GPU box except the JSON it
writes):

    python tests/golden/make_reader_golden.py [path of the reference's qa/ directory]

R1 pairs    qa/prepro_utils.py prepare + OnlineSampler._join_sents / paragraph mask (online_sampler.py:285-335) on ~10
            passages (Zs spaces, accents, truncation, an empty question, an empty passage), vocab_small.txt
R2 forward  qa/bert_retrieve_qa.py BertRetrieveQA.forward in fp32 on a small random model (--add-select), stored with its
            weights (fp16: the weights the GPU runs; the outputs are computed from exactly those) in reader_forward_golden.npz
R3 predict  qa/train_retrieve_qa.py predict() with a stub model and a stub eval_load returning given logits: the printed
            lines and the --save-pred records of every alpha (ties, a duplicated question, regex and exact match)
Modules the reference imports but this container lacks are stubbed in sys.modules (tensorflow, faiss, apex,
torch.utils.tensorboard); transformers' AdamW is stubbed too (the predict path never constructs it).
"""
import contextlib
import glob
import importlib.machinery
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/qa"


def stub_modules():
    for name in ("tensorflow", "faiss", "apex", "torch.utils.tensorboard"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            m.SummaryWriter = object
            sys.modules[name] = m
    import transformers
    try:
        from transformers import AdamW  # noqa: F401
    except ImportError:
        transformers.__dict__["AdamW"] = object   # (the lazy module ignores a plain setattr)
    sys.path.insert(0, REF)
    # bert_retrieve_qa imports the retriever's model from the sibling retrieval/ directory (after qa/: its utils wins)
    sys.path.append(os.path.join(os.path.dirname(os.path.abspath(REF)), "retrieval"))


PASSAGES = [
    "The Eiffel Tower is in Paris, France.",
    "café naïve résumé — coöperate",                 # accents (NFD'd by the sampler)
    "word with Zs　spaces and\ttabs\nnewlines\rreturns",           # Zs separators
    "unbelievable things happened in the first world war",
    " ".join(["paris"] * 80),                                                     # truncates at max_length
    "",                                                                           # empty passage
    "(1984) - 'quoted', \"double\"! what?",
    "xyzzyplughqwertyuiopasdfghjklzxcvbnm supercalifragilistic",                  # [UNK] and long words
    "the king of the new york state university school",
    "Hello    world",
]
QUESTIONS = ["who was the first king of france ?", "", "what is the capital city"]


def make_pairs(tok_dir):
    from transformers import BertTokenizer
    from prepro_utils import prepare, normalize
    from online_sampler import OnlineSampler
    tok = BertTokenizer.from_pretrained(tok_dir)
    fake = types.SimpleNamespace(tokenizer=tok)
    out = []
    for max_len in (64, 24):
        for qi, q in enumerate(QUESTIONS):
            q_ids = torch.LongTensor(tok.encode(q, max_length=12, truncation=True))
            for p in PASSAGES:
                p = normalize(normalize(p))
                doc_tokens, _, _, t2o, subtoks = prepare(p, tok)
                po = q_ids.size(0)
                keep = subtoks[:max_len - po - 1] if len(subtoks) > max_len - po - 1 else subtoks
                p_ids = torch.LongTensor(tok.convert_tokens_to_ids(keep))
                ids, seg = OnlineSampler._join_sents(fake, q_ids[1:-1], p_ids)
                mask = torch.zeros(ids.shape).bool()
                mask[po:-1] = 1
                out.append({"question": q, "passage": p, "max_seq_length": max_len, "q_ids": q_ids.tolist(),
                            "doc_tokens": doc_tokens, "tok_to_orig_index": t2o, "all_doc_tokens": subtoks,
                            "input_ids": ids.tolist(), "segment_ids": seg.tolist(),
                            "paragraph_mask": mask.long().tolist(), "para_offset": po})
    return out


def make_predict():
    import bert_retrieve_qa  # noqa: F401  (importing the model replaces sys.modules["transformers"]: stub AdamW after it)
    sys.modules["transformers"].__dict__.setdefault("AdamW", object)
    import train_retrieve_qa as T
    import hashlib
    import re
    # One batch per question; every item is (doc, span as (first piece, last piece) of the doc, span score, rank score).
    # The scores are chosen so that rank and span disagree and the top passage moves across the alphas: EM takes several
    # values.  "who wrote hamlet" is asked twice (one group of four entries); at alpha 0.5 its two leading entries tie
    # exactly (4 * 0.5 == 4 * 0.5), so the answer there depends on the order the previous alpha left (the reference sorts
    # the list in place, stably).  Answers exercise normalisation (case, articles, punctuation) and, for the year, a
    # regular-expression gold that only --regex matches.
    docs = [["William", "Shakespeare", "wrote", "Hamlet", "in", "1600."],
            ["Paris", "is", "the", "capital", "of", "France."],
            ["The", "café", "(Jupiter)", "is", "large,", "isn't", "it?"],
            ["Apollo", "11", "landed", "in", "1969", "on", "the", "Moon."]]

    def pieces_of(doc):
        wp, t2o = [], []
        for wi, w in enumerate(doc):
            ps = re.findall(r"\w+|[^\w\s]", w.lower())
            wp += ps
            t2o += [wi] * len(ps)
        return wp, t2o

    spec = [
        ("who wrote hamlet", ["william shakespeare"], [(0, (0, 1), 4.0, 0.0),       # right, wins for alpha > 0.5
                                                       (1, (0, 0), 0.0, 4.0),       # wrong, wins for alpha < 0.5
                                                       (3, (4, 4), -2.0, -2.0)]),
        ("capital of france", ["The Paris!"], [(1, (0, 0), 0.0, 2.0),              # right ("Paris"), ties at 0.25
                                               (2, (1, 1), 6.0, 0.0)]),             # "café"
        ("who wrote hamlet", ["william shakespeare"], [(0, (3, 3), 10.0, -10.0)]),  # "Hamlet": wins for alpha >= 0.7
        ("largest planet", ["the Jupiter", "jupiter planet"], [(2, (3, 3), 3.0, 1.0),   # "jupiter" out of "(Jupiter)"
                                                               (3, (0, 1), 5.0, 0.0)]),  # "Apollo 11"
        ("year of moon landing", ["19[0-9]{2}", "nineteen sixty-nine"], [(3, (4, 4), 2.0, 2.0),   # "1969"
                                                                         (0, (5, 6), 1.0, 1.0)]),  # "1600."
    ]
    batches = []
    L = 40
    po = 5
    for q, ans, items in spec:
        n_items = len(items)
        start = torch.full((n_items, L), -1e10)
        end = torch.full((n_items, L), -1e10)
        wps, t2os, dts = [], [], []
        for k, (d, (i, j), span, _) in enumerate(items):
            wp, t2o = pieces_of(docs[d])
            wps.append(wp)
            t2os.append(t2o)
            dts.append(docs[d])
            start[k, po:po + len(wp)] = -4.0
            end[k, po:po + len(wp)] = -4.0
            start[k, po + i] = span / 2
            end[k, po + j] = span / 2
        rank = torch.tensor([it[3] for it in items])
        batches.append(({"id": [hashlib.md5(q.encode()).hexdigest()] * n_items, "q": [q] * n_items, "doc_tokens": dts,
                         "wp_tokens": wps, "tok_to_orig_index": t2os, "para_offset": [po] * n_items,
                         "true_answers": [ans] * n_items, "net_input": {}},
                        {"start_logits": start, "end_logits": end, "rank_logits": rank, "select_logits": rank.view(-1, 1)}))

    class Loader:
        def __init__(self):
            self.i = 0

        def eval_load(self, retriever, k):
            for b, _ in batches:
                yield b

        def __len__(self):
            return len(batches)

    class Model:
        retriever = None

        def __init__(self):
            self.n = 0

        def eval(self):
            return self

        def train(self):
            return self

        def __call__(self, batch):
            out = batches[self.n][1]
            self.n += 1
            return out

    runs = []
    for regex in (False, True):
        with tempfile.TemporaryDirectory() as tmp:
            args = types.SimpleNamespace(eval_k=3, add_select=False, do_lower_case=True, save_all=False, regex=regex,
                                         save_pred=True, prefix=os.path.join(tmp, "pred"))
            T.move_to_cuda = lambda x: x
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
                best = T.predict(args, Model(), Loader(), "cpu", fp16=False)
            preds = {}
            for path in sorted(glob.glob(os.path.join(tmp, "pred_*.json"))):
                key = os.path.basename(path)[len("pred_"):-len(".json")]
                preds[key] = [json.loads(l) for l in open(path)]
        runs.append({"regex": regex, "lines": buf.getvalue().splitlines(), "best": float(best), "preds": preds})
    inputs = [{"batch": {k: v for k, v in b.items() if k != "net_input"},
               "start_logits": r["start_logits"].tolist(), "end_logits": r["end_logits"].tolist(),
               "rank_logits": r["rank_logits"].tolist()} for b, r in batches]
    return {"inputs": inputs, "runs": runs}


# small enough that the weights fit a committed file (< 1 MiB); hidden 128 = 2 heads of 64 (the attention kernel's head size)
FWD_CFG = dict(vocab_size=200, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128,
               max_position_embeddings=40, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")


def make_forward(tmp):
    """R2: BertRetrieveQA.forward (bert_retrieve_qa.py:58-77) of a small random model in fp32, --add-select on: the masked
    start / end logits, rank logits (q . para_embed) and select logits, with the state dict that produced them."""
    from transformers import BertConfig, BertModel
    from bert_retrieve_qa import BertRetrieveQA
    torch.manual_seed(4321)
    cfg = BertConfig(**FWD_CFG)
    BertModel(cfg).save_pretrained(tmp)
    args = types.SimpleNamespace(shared_norm=False, separate=False, add_select=True, drop_early=False, use_spanbert=False,
                                 bert_model_name=tmp, retriever_path="", qa_drop=0.0)
    model = BertRetrieveQA(cfg, args)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            v = 1.0 + 0.1 * torch.randn(prm.shape, generator=g) if name.endswith("LayerNorm.weight") else \
                0.05 * torch.randn(prm.shape, generator=g)
            prm.copy_(v.half().float())      # fp16-exact: the stored weights are the ones the outputs come from
    model.eval()
    rng = np.random.default_rng(8)
    lens, qlen = [37, 20, 29], 6
    B, L = len(lens), max(lens)
    ids = torch.zeros((B, L), dtype=torch.long)
    seg = torch.zeros((B, L), dtype=torch.long)
    pmask = torch.zeros((B, L), dtype=torch.long)
    amask = torch.zeros((B, L), dtype=torch.long)
    for b, n in enumerate(lens):
        x = torch.from_numpy(rng.integers(104, FWD_CFG["vocab_size"], n))
        x[0], x[qlen - 1], x[n - 1] = 101, 102, 102
        ids[b, :n] = x
        seg[b, qlen:n] = 1
        pmask[b, qlen:n - 1] = 1
        amask[b, :n] = 1
    q_ids = torch.from_numpy(rng.integers(104, FWD_CFG["vocab_size"], (1, qlen)))
    q_ids[0, 0], q_ids[0, -1] = 101, 102
    para_embed = torch.from_numpy(rng.standard_normal((B, 128)).astype(np.float32))
    batch = {"input_ids": ids, "input_mask": amask, "segment_ids": seg, "paragraph_mask": pmask, "input_ids_q": q_ids,
             "input_mask_q": torch.ones_like(q_ids), "para_embed": para_embed}
    with torch.no_grad():
        out = model(batch)
    # the passage tower (retriever.bert_c / proj_c) takes no part in the forward: not stored
    arrays = {f"w::{k}": v.numpy().astype(np.float16) for k, v in model.state_dict().items()
              if not k.endswith("position_ids") and not k.startswith(("retriever.bert_c.", "retriever.proj_c."))}
    arrays.update(config=np.asarray(json.dumps(FWD_CFG)),input_ids=ids.numpy(), segment_ids=seg.numpy(), seq_lens=np.asarray(lens), para_offset=np.full(B, qlen),
                  input_ids_q=q_ids.numpy(), para_embed=para_embed.numpy(),
                  start_logits=out["start_logits"].numpy(), end_logits=out["end_logits"].numpy(),
                  rank_logits=out["rank_logits"].numpy(), select_logits=out["select_logits"].numpy())
    return arrays


def main():
    stub_modules()
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(HERE, "vocab_small.txt")) as f:
            vocab = f.read()
        with open(os.path.join(tmp, "vocab.txt"), "w") as f:
            f.write(vocab)
        pairs = make_pairs(tmp)
    predict = make_predict()
    with tempfile.TemporaryDirectory() as tmp:
        fwd = make_forward(tmp)
    np.savez_compressed(os.path.join(HERE, "reader_forward_golden.npz"), **fwd)
    with open(os.path.join(HERE, "reader_golden.json"), "w") as f:
        json.dump({"pairs": pairs, "predict": predict}, f, ensure_ascii=False)
    print(f"wrote reader_golden.json: {len(pairs)} pairs, {len(predict['runs'])} predict runs")


if __name__ == "__main__":
    main()
