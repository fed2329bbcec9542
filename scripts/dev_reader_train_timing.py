"""The reader's sampling step and whole training steps at the shape of train_dense_qa.sh, on a seeded synthetic world
(developer tool): bert-base with seeded weights, 5 passages of 150-400 words per question, 12-token questions, k = 5000
over --rows seeded fp16 rows (default 18M) with the synthetic sqlite corpus of dev_reader_timing.py --cli mapped onto them
(row r is passage r mod --passages).

Measures (one JSON line, and --out FILE):
  sampling step   new route (OnlineSampler: encode, search, ONE collect launch, record down, host text for k passages, one
                  copy up) against the parent's route (encode, OnlineRetriever.retrieve with row-ordered ids -- I and the
                  rows to the host --, the host label loop, float32 rows and int64 labels back up, over the same host text
                  work).  The two take turns question by question in one process; a host clock around work that ends in a
                  synchronise; medians of --questions questions after --warmup.
  split           the sampler's per-stage seconds with a synchronise after every stage
  steps           whole training steps per second (sampler + TrainableReader forward / backward + FusedAdamW.step)
  collect kernel  device events around the collect_labeled_device call (kernel, 16-byte memset, three allocations; the
                  kernel alone is the trace's: `rocprofv3 --kernel-trace --stats -- python
                  scripts/dev_reader_train_timing.py --only-collect 200`, a run of its own), against the bytes it moves,
                  k x 256 B in and out, over 8 TB/s
  --lookahead 1,4,8   the sampling step with the questions retrieved in groups (OnlineSampler.retrieve_many: one tower pass,
                  one search, one collect launch, one record copy per group) against groups of one, which is
                  OnlineSampler.retrieve.  The contenders take turns, block of lcm(W) questions by block, in one process, the
                  first of a block rotating (it pays for the passages the block brings into the cache); a host clock from a
                  synchronise to a synchronise around the block's groups, their host text work and copies up, divided by
                  the block's questions; medians over the blocks of --questions questions after --warmup.  Then the
                  per-stage split of every contender with a synchronise after every stage (passages cached).  Only this is
                  measured, and --out receives it.  `--only-collect N --lookahead W` retrieves N questions in groups of W
                  for a trace of the collect kernel.
Transfer sizes are counted from the shapes: new route (2 + k) x 8 bytes down; parent route k x 8 + k x 512 bytes down and
k x 516 bytes up.
"""
import argparse
import json
import os
import sqlite3
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K_SEARCH = 5000


class ModuloIds:
    """row-ordered paragraph ids of a corpus mapped onto more rows than it has passages: row r -> d{r mod passages}"""

    def __init__(self, rows, passages):
        self.rows, self.passages = rows, passages

    def __len__(self):
        return self.rows

    def __getitem__(self, r):
        return f"d{r % self.passages}"

    def __iter__(self):
        # (the inverse keeps one row per paragraph id: the first `passages` rows name every id)
        return (f"d{r}" for r in range(min(self.rows, self.passages)))


def build_world(tmp, args):
    from proqa_amd.retriever import BERT_BASE
    rng = np.random.default_rng(1)
    special = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    words = [f"w{i}" for i in range(BERT_BASE["vocab_size"] - len(special))]
    model_dir = os.path.join(tmp, "model")
    os.makedirs(model_dir)
    with open(os.path.join(model_dir, "vocab.txt"), "w") as f:
        f.write("\n".join(special + words) + "\n")
    with open(os.path.join(model_dir, "config.json"), "w") as f:
        json.dump(dict(BERT_BASE, model_type="bert"), f)
    warr = np.asarray(words)
    con = sqlite3.connect(os.path.join(tmp, "docs.db"))
    con.execute("CREATE TABLE documents (id PRIMARY KEY, text)")
    con.executemany("INSERT INTO documents VALUES (?, ?)",
                    ((f"d{p}", " ".join(warr[rng.integers(0, len(words), int(rng.integers(150, 401)))]))
                     for p in range(args.passages)))
    con.commit()
    con.close()
    n_q = args.questions + args.warmup
    with open(os.path.join(tmp, "train.txt"), "w") as f, open(os.path.join(tmp, "matched.txt"), "w") as g:
        for _ in range(n_q):
            q = " ".join(warr[rng.integers(0, len(words), 10)])              # 10 words: 12 tokens
            a = str(warr[rng.integers(0, len(words))])
            f.write(json.dumps({"question": q, "answer": [a]}) + "\n")
            gold = {f"d{int(p)}": a for p in rng.integers(0, args.passages, args.gold)}
            g.write(json.dumps({"question": q, "matched_paras": gold}) + "\n")
    return model_dir


def fill_index(index, rows, device):
    g = torch.Generator(device=device).manual_seed(7)
    step = 1 << 21
    for r0 in range(0, rows, step):
        index.add_device(torch.randn((min(step, rows - r0), 128), generator=g, device=device, dtype=torch.float16))


def time_lookahead(sampler, retriever, group_sizes, args, sync, note):
    """the sampling step per question with groups of every size of group_sizes (1 is the yardstick: retrieve)"""
    import math
    block = math.lcm(*group_sizes)

    def run_block(qas, w):
        for at in range(0, len(qas), w):
            group = qas[at:at + w]
            for qa, retrieved in zip(group, sampler.retrieve_many(retriever, [qa["question"] for qa in group], args.k)):
                sampler._batch(qa, retrieved)
        sync()

    times = {w: [] for w in group_sizes}
    blocks = [sampler.qa_data[at:at + block] for at in range(0, len(sampler.qa_data) - block + 1, block)]
    warm_blocks = -(-args.warmup // block)
    for n, qas in enumerate(blocks):
        turn = n % len(group_sizes)
        for w in group_sizes[turn:] + group_sizes[:turn]:
            sync()
            t0 = time.perf_counter()
            run_block(qas, w)
            dt = time.perf_counter() - t0
            if n >= warm_blocks:
                times[w].append(dt / len(qas))
    med = {w: statistics.median(v) * 1e3 for w, v in times.items()}
    note(f"sampling step per question, medians by group size: {med}")

    # the per-stage split, a synchronise after every stage (passages now cached: host_text is the cached figure)
    sampler.sync_stages = True
    split = {}
    for w in group_sizes:
        for key in sampler.seconds:
            sampler.seconds[key] = 0.0
        n_split = 0
        for qas in blocks[warm_blocks:]:
            run_block(qas, w)
            n_split += len(qas)
        split[w] = {k: round(v / n_split * 1e3, 3) for k, v in sampler.seconds.items()}
    sampler.sync_stages = False
    note("split done")
    return {
        "rows": args.rows, "k_search": K_SEARCH, "k": args.k, "gold_rows": args.gold, "block_questions": block,
        "questions": (len(blocks) - warm_blocks) * block, "blocks": len(blocks) - warm_blocks,
        "yardstick": "groups of one: OnlineSampler.retrieve, one question at a time",
        "sampling_ms_per_question_median": {str(w): round(v, 3) for w, v in med.items()},
        "sampling_ms_per_question_p10_p90": {str(w): [round(float(np.percentile(v, 10)) * 1e3, 3),
                                                      round(float(np.percentile(v, 90)) * 1e3, 3)] for w, v in times.items()},
        "questions_per_second_sampler_bound": {str(w): round(1e3 / v, 1) for w, v in med.items()},
        "split_ms_per_question_synced": {str(w): v for w, v in split.items()},
        "collect_kernel_us": "not measured here: rocprofv3 --kernel-trace --stats, a run of its own with --only-collect",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=18_000_000)
    ap.add_argument("--passages", type=int, default=20000)
    ap.add_argument("--questions", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--gold", type=int, default=1000, help="matched paragraphs per question")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40, help="whole training steps to time (0: skip)")
    ap.add_argument("--only-collect", type=int, default=0, help="run this many sampler retrievals and exit (for a trace)")
    ap.add_argument("--lookahead", type=str, default="", help="comma-separated group sizes, e.g. 1,4,8: time the sampling "
                    "step in groups against groups of one, and nothing else")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    group_sizes = sorted({int(w) for w in args.lookahead.split(",") if w.strip()} | ({1} if args.lookahead else set()))
    if any(w < 1 for w in group_sizes):
        ap.error("--lookahead: group sizes must be >= 1")
    from transformers import BertTokenizer
    from proqa_amd.index import IndexFlatIP
    from proqa_amd.online_retriever import OnlineRetriever
    from proqa_amd.online_sampler import OnlineSampler
    from proqa_amd.optim import FusedAdamW
    from proqa_amd.pretrain_retriever import parameter_groups
    from proqa_amd.qa_utils import hash_question
    from proqa_amd.reader import random_state_dict
    from proqa_amd.retriever import BERT_BASE
    from proqa_amd.trainable_reader import TrainableReader
    from proqa_amd.utils import DocDB

    dev = torch.device("cuda", torch.cuda.current_device())
    sync = torch.cuda.synchronize

    def note(text):
        print(f"[{time.strftime('%H:%M:%S')}] {text}", file=sys.stderr, flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        model_dir = build_world(tmp, args)
        note("world written")
        tokenizer = BertTokenizer.from_pretrained(model_dir)
        index = IndexFlatIP(128, capacity=args.rows)
        fill_index(index, args.rows, dev)
        note("index filled")
        ids_of = ModuloIds(args.rows, args.passages)
        model = TrainableReader(BERT_BASE, dev, shared_norm=True, qa_drop=0.1, hidden_dropout_prob=0.1,
                                attention_probs_dropout_prob=0.1, dropout_seed=3)
        model.load_state_dict(random_state_dict(BERT_BASE, seed=0))
        model.freeze_c_encoder()
        model.train()
        sampler = OnlineSampler(os.path.join(tmp, "train.txt"), tokenizer, 12, 512, DocDB(os.path.join(tmp, "docs.db")), index,
                                index2paraid=ids_of, matched_para_path=os.path.join(tmp, "matched.txt"), device=dev)
        retriever = model.retriever
        note("model and sampler built")

        if args.only_collect:
            w = max(group_sizes, default=1)
            todo = sampler.qa_data[:args.only_collect]
            for at in range(0, len(todo), w):
                sampler.retrieve_many(retriever, [qa["question"] for qa in todo[at:at + w]], args.k)
            sync()
            return

        if group_sizes:
            result = time_lookahead(sampler, retriever, group_sizes, args, sync, note)
            print(json.dumps(result))
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
            return

        parent = OnlineRetriever(np.float16, index2paraid=ids_of, device=dev, index=index)

        def new_route(qa):
            q_ids, para_embed, labels, n_live, n_gold, top_rows = sampler.retrieve(retriever, qa["question"], args.k)
            preps = sampler._prepared(top_rows)
            spans = [sampler._spans(p, qa["answer"]) for p in preps]
            batch = sampler._collate(qa, q_ids, preps, spans)
            batch["net_input"]["para_embed"], batch["net_input"]["top5000_labels"] = para_embed, labels
            sync()
            return batch

        def parent_route(qa):
            q_ids = tokenizer.encode(qa["question"], max_length=12, truncation=True)
            with torch.no_grad():
                ids = torch.tensor([q_ids], dtype=torch.int64, device=dev)
                retriever.eval()
                q = retriever.get_embed({"input_ids": ids, "input_mask": torch.ones_like(ids, dtype=torch.bool)}, True)["embed"]
                retriever.train()
            para_embed_idx, para_idx, para_embeds = parent.retrieve(q, K_SEARCH)
            gold = sampler.qid2goldparas[hash_question(qa["question"])]
            labels = [int(p in gold) for p in para_idx]
            preps = sampler._prepared(para_embed_idx[:args.k].tolist())
            spans = [sampler._spans(p, qa["answer"]) for p in preps]
            batch = sampler._collate(qa, q_ids, preps, spans)
            batch["net_input"]["para_embed"] = torch.from_numpy(para_embeds.astype("float32")).to(dev)
            batch["net_input"]["top5000_labels"] = torch.LongTensor(labels).to(dev)
            sync()
            return batch

        times = {"new": [], "parent": []}
        for n, qa in enumerate(sampler.qa_data):
            order = (("new", new_route), ("parent", parent_route)) if n % 2 == 0 else (("parent", parent_route), ("new", new_route))
            for name, route in order:
                sync()
                t0 = time.perf_counter()
                route(qa)
                dt = time.perf_counter() - t0
                if n >= args.warmup:
                    times[name].append(dt)
        med = {k: statistics.median(v) * 1e3 for k, v in times.items()}
        note(f"sampling medians {med}")

        # the per-stage split, a synchronise after every stage (passages now cached: host_text is the cached figure)
        sampler.sync_stages = True
        for key in sampler.seconds:
            sampler.seconds[key] = 0.0
        n_split = 0
        for batch in sampler.load(retriever, k=args.k):
            n_split += 1
        sync()
        split = {k: v / n_split * 1e3 for k, v in sampler.seconds.items()}
        sampler.sync_stages = False
        note("split done")

        # the collect_labeled_device call, device events
        q = torch.randn((1, 128), device=dev, dtype=torch.float16)
        _, I = index.search_device(q, K_SEARCH)
        gold = torch.sort(torch.randperm(args.rows, device=dev)[:args.gold])[0]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(5):
            index.collect_labeled_device(I.reshape(-1), gold, args.k)
        reps = 200
        ev[0].record()
        for _ in range(reps):
            index.collect_labeled_device(I.reshape(-1), gold, args.k)
        ev[1].record()
        sync()
        collect_us = ev[0].elapsed_time(ev[1]) / reps * 1e3      # (includes the 16-byte memset and three allocations)
        collect_bytes = 2 * K_SEARCH * 256

        steps_per_s = None
        if args.steps:
            opt = FusedAdamW(parameter_groups(model, 0.0), lr=1e-5, max_grad_norm=5.0, loss_scale="dynamic")
            done, t0 = 0, None
            for batch in sampler.load(retriever, k=args.k):
                if not batch:
                    continue
                if done == 5:
                    sync()
                    t0 = time.perf_counter()
                out = model(batch["net_input"])
                opt.scale_loss(out["loss"]).backward()
                opt.step()
                model.zero_grad()
                done += 1
                if done == 5 + args.steps:
                    break
            sync()
            if t0 is not None and done > 5:
                steps_per_s = (done - 5) / (time.perf_counter() - t0)

        result = {
            "rows": args.rows, "k_search": K_SEARCH, "k": args.k, "questions": len(times["new"]), "gold_rows": args.gold,
            "sampling_ms_median": {"new": round(med["new"], 3), "parent": round(med["parent"], 3)},
            "sampling_ms_p10_p90": {k: [round(float(np.percentile(v, 10)) * 1e3, 3), round(float(np.percentile(v, 90)) * 1e3, 3)]
                                    for k, v in times.items()},
            "split_ms_per_question_synced": {k: round(v, 3) for k, v in split.items()},
            "collect_launch_us_events": round(collect_us, 2),
            "collect_bytes": collect_bytes, "collect_us_at_8TBps": round(collect_bytes / 8e12 * 1e6, 3),
            "train_steps_per_second": None if steps_per_s is None else round(steps_per_s, 2),
            "transfer_bytes": {"new_d2h": (2 + args.k) * 8, "parent_d2h": K_SEARCH * 8 + K_SEARCH * 512,
                               "parent_h2d": K_SEARCH * 516},
            "transfers": dict(sampler.transfers),
        }
        print(json.dumps(result))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
