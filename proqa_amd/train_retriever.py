"""`python train_retriever.py --do_predict --predict_file dev.txt --init_checkpoint ckpt.pt`: the retriever's own dev
metric (/root/reference/retrieval/train_retriever.py main :100-135 + :287-290, predict :293-333) on MI355X.

Every (Question, Paragraph) pair of the dev file goes through both towers in batches of --predict_batch_size; within a
batch every question is scored against every paragraph, and the metric is how often a question's own paragraph scores
highest.  Same flags (proqa_amd.config), same two printed lines.  The reference forms `q @ c.T` and its argmax per
batch; here proqa_inbatch_eval_f16 gives the argmax, the rank of the gold paragraph and the softmax statistics of the
batch without forming the product, and the host reads them once, after the last batch.

Intended differences: the accuracy is a Python float holding the reference's float32 quotient (the reference returns and
prints a 0-d tensor, whose repr names its device); --efficient_eval changes nothing (the towers run in fp16 either way);
the mean in-batch loss and MRR are not printed but written, with the timings, to the file PROQA_STATS_JSON names.  Training (--do_train) and the `;` ensemble list of
--init_checkpoint (which the reference's own predict cannot run either: a list has no .eval()) are refused.
"""
import json
import os
import random
import time

LAST_RUN_STATS = {}


def _refuse(args):
    if not args.do_train and not args.do_predict:
        raise ValueError("At least one of `do_train` or `do_predict` must be True.")
    if args.do_train:
        raise SystemExit("train_retriever.py: --do_train is not supported: this project runs the retriever's "
                         "evaluation (--do_predict) only; train with the reference.")
    if not args.predict_file:
        raise ValueError("If `do_predict` is True, then `predict_file` must be specified.")
    if ";" in args.init_checkpoint:
        raise SystemExit("train_retriever.py: a ';' list in --init_checkpoint (the reference's ensemble path) is not "
                         "supported; evaluate one checkpoint at a time.")
    if args.init_checkpoint == "":
        raise SystemExit("train_retriever.py: --do_predict needs --init_checkpoint (an untrained retriever has no dev metric)")
    if args.no_cuda:
        raise RuntimeError("--no_cuda: proqa_amd has no CPU path")


def predict(args, model, eval_dataloader, device, fp16=False, stats=None):
    """The reference's predict: one in-batch comparison per collated batch (the short last batch included), accuracy =
    correct / total over the whole file.  Prints the reference's two lines and returns the accuracy as a float.
    A batch may carry the host lists 'seq_lens_q' / 'seq_lens_c' (ReTokenizeCollate); one of re_collate's shape has its
    masks checked on the device.  stats (optional dict) receives examples, correct, acc, loss, mrr and the encode /
    score seconds."""
    import numpy as np
    import torch
    from .inbatch import inbatch_eval
    from .utils import move_to_cuda
    model.eval()
    num_total = 0.0
    parts = []          # per batch: device [3] = (correct, sum of lse - gold, sum of 1 / (rank + 1))
    t_encode = t_score = 0.0
    for batch in eval_dataloader:
        lens_q = batch.pop("seq_lens_q", None) if isinstance(batch, dict) else None
        lens_c = batch.pop("seq_lens_c", None) if isinstance(batch, dict) else None
        t0 = time.perf_counter()
        batch_to_feed = move_to_cuda(batch, device)
        with torch.no_grad():
            if lens_q is not None and lens_c is not None:
                results = model(batch_to_feed, check_mask=False, seq_lens_q=lens_q, seq_lens_c=lens_c)
            else:
                results = model(batch_to_feed)
            t1 = time.perf_counter()
            out = inbatch_eval(results["q"], results["c"])
            n = out["argmax"].shape[0]
            target = torch.arange(n, device=out["argmax"].device, dtype=torch.int32)
            parts.append(torch.stack([(out["argmax"] == target).sum().to(torch.float64),
                                      (out["lse"] - out["gold"]).sum(dtype=torch.float64),
                                      (1.0 / (out["rank"].to(torch.float64) + 1.0)).sum()]))
        num_total += n
        t_encode += t1 - t0
        t_score += time.perf_counter() - t1
    t2 = time.perf_counter()
    sums = torch.stack(parts).sum(0).cpu().tolist() if parts else [0.0, 0.0, 0.0]     # the one host copy
    t_score += time.perf_counter() - t2     # (waits for every batch: the launches above are asynchronous)
    num_correct = float(sums[0])
    # (the reference's num_correct is a float32 tensor: its quotient is a float32 one)
    acc = float(np.float32(num_correct) / np.float32(num_total))
    print(f"evaluated {num_total} examples...")
    print(f"avg. Acc: {acc}")
    if stats is not None:
        stats.update(examples=int(num_total), correct=int(num_correct), acc=acc, loss=sums[1] / num_total,
                     mrr=sums[2] / num_total, seconds={"encode": t_encode, "score": t_score})
    model.train()
    return acc


def main(argv=None):
    from .config import get_args
    args = get_args(argv)
    if args.accumulate_gradients < 1:
        raise ValueError("Invalid accumulate_gradients parameter: {}, should be >= 1".format(args.accumulate_gradients))
    _refuse(args)
    import numpy as np
    import torch
    from transformers import BertTokenizer
    from .datasets import ReDataset, ReTextView, ReTokenizeCollate
    from .get_embed import load_bert_config, load_saved, usable_cpus
    from .retriever import BertForRetriever

    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: the retriever evaluation has no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)

    t_start = time.perf_counter()
    bert_config = load_bert_config(args.bert_model_name)
    model = BertForRetriever(bert_config, args, device=device)
    tokenizer = BertTokenizer.from_pretrained(args.bert_model_name)
    eval_dataset = ReDataset(tokenizer, args.predict_file, args.max_query_length, args.max_seq_length)
    if len(eval_dataset) == 0:
        raise ValueError(f"{args.predict_file} holds no example")
    # whole batches of (question, paragraph) strings, tokenised per side (native WordPiece for plain sentences on
    # --eval-workers threads, the tokenizer itself for the rest): the tensors of ReDataset + re_collate
    texts = ReTextView(eval_dataset)
    workers = max(0, min(args.eval_workers, usable_cpus() - 2))
    collate = ReTokenizeCollate(tokenizer, args.max_query_length, args.max_seq_length, native_threads=workers)
    n = len(texts)
    eval_dataloader = (collate([texts[i] for i in range(b0, min(b0 + args.predict_batch_size, n))])
                       for b0 in range(0, n, args.predict_batch_size))
    model = load_saved(model, args.init_checkpoint)
    model.to(device)
    model.half()
    t_loaded = time.perf_counter()

    stats = LAST_RUN_STATS
    stats.clear()
    acc = predict(args, model, eval_dataloader, device, fp16=args.efficient_eval, stats=stats)
    print(acc)
    stats["seconds"]["load"] = t_loaded - t_start
    if os.environ.get("PROQA_STATS_JSON"):
        with open(os.environ["PROQA_STATS_JSON"], "w") as f:
            json.dump(stats, f)
    return acc


if __name__ == "__main__":
    main()
