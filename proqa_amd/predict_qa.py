"""`python train_retrieve_qa.py --do_predict ...`: the reference's open-domain QA evaluation (qa/train_retrieve_qa.py
predict :274-401 over OnlineSampler.eval_load, qa/online_sampler.py:266-335) on MI355X.

Same command line, same printed lines in the same order.  Where the reference runs one question at a time, this runs
    1. the question tower over all questions (batches of 256),
    2. one top-eval_k search of the index: exact inner product by default (--search exact), or the reference's own
       IVF-Flat (--search ivf: nlist 100 / nprobe 20, L2 inside the probed lists, qa/online_sampler.py:75-79),
    3. pair building on the host: every retrieved passage once, all its words WordPiece'd in one native batch,
    4. the reader over packed batches of up to --reader-batch sequences (proqa_encoder_forward_hidden +
       proqa_reader_span_f16: the best span of each sequence comes back, never the [B, L, L] score tensor),
    5. answer texts and the alpha sweep on the host.
With --n-best N (not in the reference) step 4 runs proqa_reader_span_nbest_f16 instead -- the N best spans of every
sequence and its two log-partitions, still one launch per batch -- and after the unchanged alpha sweep one more line
reports the EM of marginal decoding (qa_utils.marginal_answers: an answer's probability summed over its mentions in all
of the question's passages, normalised per --marginal).
The rank score of a passage is its fp32 dot product with the fp16 question embedding (the search score of the exact
index; under --search ivf the inner product the IVF search returns beside its L2 distance, as the reference's rank_logits
is q . para_embed of the gathered rows, qa/bert_retrieve_qa.py:76); under --efficient_eval the reference rounds it to
fp16.  A passage without any paragraph token gets the answer ""
(the reference raises IndexError there).  Training (--do_train) is refused here: it is train_reader.py, whose dev
evaluation is this module's evaluate().
"""
import argparse
import json
import os
import sys
import time

import numpy as np

TRAINING_FLAGS = ("--do_train", "--train_file", "--raw-train-data", "--learning_rate", "--train_batch_size",
                  "--num_train_epochs", "--shared-norm", "--separate", "--use-spanbert", "--fp16", "--retriever-path",
                  "--matched-para-path", "--fix-para-encoder", "--MI", "--drop-early", "--save-all")

LAST_RUN_STATS = {}
N_BEST_MAX = 32       # proqa_reader_span_nbest_f16's limit


def build_parser():
    p = argparse.ArgumentParser(description="ProQA reader evaluation (--do_predict) on MI355X")
    p.add_argument("--do_predict", action="store_true")
    p.add_argument("--raw-eval-data", type=str, default="../data/nq-dev.txt")
    p.add_argument("--init_checkpoint", type=str, default="")
    p.add_argument("--index-path", type=str, default="retrieval/index_data/para_embed_100k.npy")
    p.add_argument("--db-path", type=str, default="../data/nq_paras.db")
    p.add_argument("--index2paraid", type=str, default="retrieval/index_data/idx_id.json",
                   help="idx_id.json of the index (the reference's OnlineSampler default)")
    p.add_argument("--eval-k", type=int, default=5)
    p.add_argument("--max_seq_length", type=int, default=512)
    p.add_argument("--max_query_length", type=int, default=50)
    p.add_argument("--bert_model_name", type=str, default="bert-base-uncased")
    p.add_argument("--do_lower_case", action="store_true", default=True)
    p.add_argument("--efficient_eval", action="store_true",
                   help="accepted for compatibility: the reader always runs in fp16 here")
    p.add_argument("--regex", action="store_true")
    p.add_argument("--add-select", action="store_true")
    p.add_argument("--save-pred", action="store_true")
    p.add_argument("--prefix", type=str, default="eval")
    p.add_argument("--max_answer_len", type=int, default=20, help="ignored, as in the reference (spans of <= 10 pieces)")
    p.add_argument("--predict_batch_size", type=int, default=100, help="ignored (the reference runs one question at a time)")
    p.add_argument("--eval-workers", type=int, default=16, help="threads of the native WordPiece tokenizer")
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--output_dir", type=str, default="logs")
    p.add_argument("--reader-batch", type=int, default=256, help="sequences per reader launch (not in the reference)")
    p.add_argument("--search", choices=("exact", "ivf"), default="exact",
                   help="exact inner-product search (default), or the reference's IndexIVFFlat (L2 lists behind an "
                        "inner-product quantizer, qa/online_sampler.py:75-79; not in the reference's command line)")
    p.add_argument("--nlist", type=int, default=100, help="--search ivf: inverted lists (the reference's 100)")
    p.add_argument("--nprobe", type=int, default=20, help="--search ivf: lists probed per question (the reference's 20)")
    p.add_argument("--n-best", type=int, default=0,
                   help="spans per passage for marginal answer decoding, 1..32; 0 = off (not in the reference)")
    p.add_argument("--marginal", choices=("shared", "passage"), default="shared",
                   help="--n-best: span probabilities normalised over all passages of a question, as --shared-norm trains "
                        "them (default), or per passage")
    return p


def check_search_args(args):
    """Refuses --n-best / --search ivf settings the kernels cannot run, before any GPU work."""
    if not 0 <= getattr(args, "n_best", 0) <= N_BEST_MAX:
        raise SystemExit(f"--n-best {args.n_best} outside [0, {N_BEST_MAX}]")
    if args.search != "ivf":
        return
    from .index import IVF_MAX_K
    if not 1 <= args.eval_k <= IVF_MAX_K:
        raise SystemExit(f"--search ivf: --eval-k {args.eval_k} outside [1, {IVF_MAX_K}] (--search exact takes any k)")
    if args.nprobe < 1:
        raise SystemExit(f"--search ivf: --nprobe {args.nprobe} < 1")
    if args.nlist < 1:
        raise SystemExit(f"--search ivf: --nlist {args.nlist} < 1")


def _refuse_training(argv):
    for a in argv:
        flag = a.split("=", 1)[0]
        if flag in TRAINING_FLAGS:
            raise SystemExit(f"train_retrieve_qa.py: {flag} is not supported: this project runs the reader's "
                             "evaluation (--do_predict) only; train with the reference.")


def load_qa(path):
    with open(path) as f:
        return [json.loads(line) for line in f.readlines()]


def evaluate(args, reader, tokenizer, qa_data, index, index2paraid, stats=None, say=print):
    """Steps 1-5 of the module's docstring over loaded pieces: reader (a BertReader), the questions of qa_data, an index that
    holds the rows (IndexFlatIP, or IndexIVFFlat under args.search == "ivf") and its idx_id.json mapping.  Prints the alpha
    sweep's lines through `say`, fills the per-stage seconds into `stats`, returns the best EM.  Also the dev evaluation of
    train_reader.py, over the index its sampler searches.  args.n_best > 0 (absent = 0): one more line after the sweep, the
    EM of marginal decoding under args.marginal (absent = "shared"), and stats["marginal_em"]; the return value stays the
    sweep's."""
    import torch
    from . import qa_utils as qu
    from .datasets import TokenizeCollate
    from .utils import DocDB
    stats = {} if stats is None else stats
    dev = reader.device
    n_best, norm = int(getattr(args, "n_best", 0) or 0), getattr(args, "marginal", "shared")
    # 1 + 2: all questions through the question tower, one search
    t0 = time.perf_counter()
    questions = [qa["question"] for qa in qa_data]
    q_ids = [tokenizer.encode(q, max_length=args.max_query_length, truncation=True) for q in questions]
    collate = TokenizeCollate(tokenizer, args.max_query_length)
    embeds = []
    for b0 in range(0, len(questions), 256):
        batch = collate(questions[b0:b0 + 256])
        embeds.append(reader.retriever.get_embed({"input_ids": batch["input_ids"].to(dev),
                                                  "input_mask": batch["input_mask"].to(dev)}, True, check_mask=False,
                                                 seq_lens_host=batch["seq_lens"])["embed"].float())
    q_embed = torch.cat(embeds).cpu().numpy() if embeds else np.zeros((0, 128), np.float32)
    if args.search == "ivf":
        t_ivf = time.perf_counter()
        _, I, D = index.search(q_embed, args.eval_k, inner_products=True)     # D: the rank score q . x
        stats["ivf_search_seconds"] = time.perf_counter() - t_ivf
        stats["ivf_search_stats"] = index.last_stats()
    else:
        D, I = index.search(q_embed, args.eval_k)
    t1 = time.perf_counter()

    # 3: pair building -- every retrieved passage once
    rows = sorted({int(r) for r in I.reshape(-1).tolist() if r >= 0})
    with DocDB(args.db_path) as db:
        texts = [qu.normalize(qu.normalize(db.get_doc_text(index2paraid[str(r)]))) for r in rows]
    wp = qu.WordPieces(tokenizer, threads=args.eval_workers)
    prepared = dict(zip(rows, qu.prepare_many(texts, wp)))
    cls_id, sep_id = tokenizer.convert_tokens_to_ids("[CLS]"), tokenizer.convert_tokens_to_ids("[SEP]")
    items = []      # (question index, row, rank score, ids, segments, para_offset)
    for qi in range(len(questions)):
        for r, d in zip(I[qi].tolist(), D[qi].tolist()):
            if r < 0:
                continue
            ids, seg, po, _ = qu.build_pair(q_ids[qi], prepared[r]["piece_ids"], args.max_seq_length, cls_id, sep_id)
            items.append((qi, r, d, ids, seg, po))
    t2 = time.perf_counter()

    # 4: the reader over packed batches
    spans, selects, nbest = [], [], []
    for b0 in range(0, len(items), args.reader_batch):
        chunk = items[b0:b0 + args.reader_batch]
        L = max(len(it[3]) for it in chunk)
        ids = np.zeros((len(chunk), L), np.int64)
        seg = np.zeros((len(chunk), L), np.int64)
        for k, it in enumerate(chunk):
            ids[k, :len(it[3])] = it[3]
            seg[k, :len(it[4])] = it[4]
        out = reader.forward({"input_ids": torch.from_numpy(ids).to(dev), "segment_ids": torch.from_numpy(seg).to(dev),
                              "seq_lens": [len(it[3]) for it in chunk], "para_offset": [it[5] for it in chunk]},
                             n_best=n_best)
        if n_best:
            nbest.append(torch.cat([out["nbest_start"], out["nbest_end"], out["nbest_score"].view(torch.int32),
                                    out["span_lse"].view(torch.int32)], 1))
        spans.append(torch.stack([out["start"], out["end"], out["span_score"].view(torch.int32)], 1))
        if out["select"] is not None:
            selects.append(out["select"])
    spans = torch.cat(spans).cpu().numpy() if spans else np.zeros((0, 3), np.int32)
    selects = torch.cat(selects).cpu().numpy().tolist() if selects else None
    nbest = torch.cat(nbest).cpu().numpy() if nbest else np.zeros((0, 3 * n_best + 2), np.int32)   # starts, ends, scores, lse
    t3 = time.perf_counter()

    # 5: texts, grouping by question hash, alpha sweep
    qid2results, qid2ground, qid2passages = {}, {}, {}
    scores = spans[:, 2].copy().view(np.float32).tolist()
    if n_best:
        nb_score = nbest[:, 2 * n_best:3 * n_best].copy().view(np.float32)
        nb_lse = nbest[:, 3 * n_best:].copy().view(np.float32)
    for n, (qi, r, d, _, _, po) in enumerate(items):
        p = prepared[r]
        text = qu.answer_text(int(spans[n, 0]), int(spans[n, 1]), po, p["doc_tokens"], p["all_doc_tokens"],
                              p["tok_to_orig_index"], args.do_lower_case)
        qid = qu.hash_question(questions[qi])
        qid2results.setdefault(qid, []).append({
            "text": text, "rank_score": selects[n] if args.add_select else d,
            "span_score": scores[n] if spans[n, 0] >= 0 else None,
            "passage": " ".join(p["doc_tokens"]), "question": questions[qi]})
        qid2ground[qid] = qa_data[qi]["answer"]
        if n_best:
            cand = [(text if k == 0 else
                     qu.answer_text(int(nbest[n, k]), int(nbest[n, n_best + k]), po, p["doc_tokens"], p["all_doc_tokens"],
                                    p["tok_to_orig_index"], args.do_lower_case), float(nb_score[n, k]))
                    for k in range(n_best) if nbest[n, k] >= 0]
            qid2passages.setdefault(qid, []).append({"rank_score": selects[n] if args.add_select else d,
                                                     "lse": nb_lse[n].tolist(), "candidates": cand})
    _, best = qu.alpha_sweep(qid2results, qid2ground, regex=args.regex,
                             save_prefix=args.prefix if args.save_pred else None, out=say)
    if n_best:
        match_fn = qu.regex_match_score if args.regex else qu.exact_match_score
        ems, saved = [], {}
        for qid, passages in qid2passages.items():
            answers = qu.marginal_answers(passages, norm)
            top = answers[0]["text"] if answers else ""
            ems.append(qu.metric_max_over_ground_truths(match_fn, top, qid2ground[qid]))
            saved[qid] = [{"answer": a["text"], "prob": a["prob"]} for a in answers[:n_best]]
        stats["marginal_em"] = float(np.mean(ems)) if ems else 0.0
        say(f"marginal (n-best {n_best}, {norm} norm): avg. EM: {stats['marginal_em']}")
        if args.save_pred:
            with open(f"{args.prefix}_marginal.json", "w") as g:
                json.dump(saved, g)
    t4 = time.perf_counter()
    stats.update(questions=len(questions), sequences=len(items), tokens=int(sum(len(it[3]) for it in items)),
                 search_seconds=t1 - t0, pair_building_seconds=t2 - t1, reader_seconds=t3 - t2, postprocess_seconds=t4 - t3)
    return best


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    _refuse_training(argv)
    args = build_parser().parse_args(argv)
    if not args.do_predict:
        raise SystemExit("train_retrieve_qa.py: only --do_predict is supported")
    check_search_args(args)
    import torch
    from transformers import BertTokenizer
    from .get_embed import load_bert_config
    from .index import IndexFlatIP, IndexIVFFlat
    from .reader import BertReader

    t_start = time.perf_counter()
    stats = LAST_RUN_STATS
    stats.clear()
    cfg = load_bert_config(args.bert_model_name)
    tokenizer = BertTokenizer.from_pretrained(args.bert_model_name)
    dev = torch.device("cuda", torch.cuda.current_device())
    reader = BertReader.load(args.init_checkpoint, cfg, dev)
    if args.add_select and not reader.add_select:
        raise SystemExit("--add-select: the checkpoint has no select_outputs")
    reader.add_select = bool(args.add_select)
    qa_data = load_qa(args.raw_eval_data)
    with open(args.index2paraid) as f:
        index2paraid = json.load(f)
    para_embed = np.load(args.index_path).astype("float32")
    if args.search == "ivf":
        # qa/online_sampler.py:75-79, and no IndexFlatIP of the rows beside it
        rows16 = torch.from_numpy(para_embed).to(dev)
        rows16 = rows16.half() if torch.equal(rows16.half().float(), rows16) else rows16
        del para_embed
        index = IndexIVFFlat(IndexFlatIP(128), 128, args.nlist)
        t_ivf = time.perf_counter()
        index.train(rows16)
        torch.cuda.synchronize()
        stats["ivf_train_seconds"] = time.perf_counter() - t_ivf
        t_ivf = time.perf_counter()
        index.add(rows16)
        torch.cuda.synchronize()
        stats["ivf_add_seconds"] = time.perf_counter() - t_ivf
        index.nprobe = args.nprobe
        del rows16
    else:
        index = IndexFlatIP(128)
        index.add(para_embed)

    t0 = time.perf_counter()
    best = evaluate(args, reader, tokenizer, qa_data, index, index2paraid, stats)
    print(best)
    t4 = time.perf_counter()
    stats.update(startup_seconds=t0 - t_start, total_seconds=t4 - t_start)
    if os.environ.get("PROQA_STATS_JSON"):
        with open(os.environ["PROQA_STATS_JSON"], "w") as f:
            json.dump(stats, f)
    return best


if __name__ == "__main__":
    main()
