"""Generate tests/golden/matched_golden.json by running the REFERENCE's own process_qa_para / para_has_answer / regex_match
(qa/prepro_dense.py) on CPU over tests/golden/recall_docs.db.

Run in the build container only (needs the reference checkout; only the .json it writes travels):

    python tests/golden/make_matched_golden.py [path of the reference's qa/ directory]

The reference's init() is never called (it fetches a tokenizer from the network and opens a hard-coded DB path): the module
globals PROCESS_TOK / PROCESS_DB are set here.  Modules the reference imports but the container lacks are stubbed, as in
make_reader_loss_golden.py.  What runs is process_qa_para (:76-92) per (question, retrieved) pair, in input order, and the
coverage line of process_ground_paras (:142-143).

Cases: the questions and documents of recall_golden.json with every document retrieved, in a seeded order per question, cut
at k = 15 of 20 (string mode); five regex questions, one of them with a pattern that does not compile (regex mode; the order
of the reference's list(set(...)) is arbitrary, so the matches are stored sorted).
"""
import importlib
import importlib.machinery
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/qa"
K = 15

REGEX_QAS = [
    {"question": "which paris", "answer": ["Par[a-z]+"]},
    {"question": "a year", "answer": ["19\\d\\d|2003"]},
    {"question": "who", "answer": ["washington( washington)?"]},
    {"question": "broken pattern", "answer": ["[unclosed("]},
    {"question": "languages", "answer": ["C\\+\\+|[CF]#"]},
]


def stub_modules():
    for name in ("tensorflow", "faiss", "apex", "tqdm", "transformers"):
        try:
            importlib.import_module(name)
        except Exception:
            m = types.ModuleType(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            m.tqdm = lambda it, **kw: it
            m.BertTokenizer = object
            sys.modules[name] = m
    sys.path.insert(0, REF)


def run(ref, qas, retrieved, match):
    lines = [ref.process_qa_para((dict(qa), result), k=K, match=match) for qa, result in zip(qas, retrieved)]
    if match == "regex":
        for line in lines:
            line["matched_paras"] = {k: sorted(v) for k, v in line["matched_paras"].items()}
    coverage = str(np.mean([len(r["matched_paras"]) > 0 for r in lines]))
    # json round trip: what the reference's json.dumps writes and a reader of the file gets back
    return {"k": K, "raw": qas, "retrieved": retrieved, "lines": json.loads(json.dumps(lines)), "coverage": coverage}


def main():
    stub_modules()
    import prepro_dense as ref
    from basic_tokenizer import SimpleTokenizer
    from utils import DocDB
    ref.PROCESS_TOK = SimpleTokenizer()
    ref.PROCESS_DB = DocDB(os.path.join(HERE, "recall_docs.db"))
    with open(os.path.join(HERE, "recall_golden.json")) as f:
        gold = json.load(f)
    doc_ids = [d[0] for d in gold["docs"]]
    rng = np.random.default_rng(11)

    def retrieved_for(qas):
        out = []
        for _ in qas:
            order = [doc_ids[i] for i in rng.permutation(len(doc_ids))]
            out.append({"para_id": order + order[:2]})      # (repeats beyond k: never read)
        out[0]["para_id"] = out[0]["para_id"][:7]           # a list shorter than k
        out[1]["para_id"][3] = out[1]["para_id"][0]         # a repeated id inside the top k
        return out

    out = {"string": run(ref, gold["qas"], retrieved_for(gold["qas"]), "string"),
           "regex": run(ref, REGEX_QAS, retrieved_for(REGEX_QAS), "regex")}
    with open(os.path.join(HERE, "matched_golden.json"), "w") as f:
        json.dump(out, f)
    for mode, case in out.items():
        print(mode, "coverage", case["coverage"], "matched", sum(len(r["matched_paras"]) for r in case["lines"]))


if __name__ == "__main__":
    main()
