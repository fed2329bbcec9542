"""Several questions per pass against one question per pass, at the shape of train_dense_qa.sh (developer tool): bert-base
with seeded weights, 5 sequences of 200-512 tokens per question (a question part of 12 tokens), P = 5000 fp16 passage
embeddings, A = 8 answer slots; synthetic net_inputs, no sampler.  One MI355X, one process; the contenders take turns
iteration by iteration; device events around each, median of --repeats (50) after --warmup (5).

Measures (one JSON line, and --out FILE):
  (a) loss        forward + backward of ONE reader_loss_multi call against a loop of Q reader_loss calls (the route of one
                  question per pass) on the same hidden states, Q = 1, 4, 8, 16
  (b) pass        questions per second of TrainableReader forward + backward with one FusedAdamW.step per 8 questions: the
                  dict route (one question per pass), and lists of 4 and of 8.  The dict route is measured three times; the
                  spread of the three is the yardstick for what counts as a difference.
Kernel times are not taken here: `rocprofv3 --kernel-trace --stats -- python scripts/dev_reader_multi_timing.py --only-loss 8
--route multi` (a run of its own; `--route loop` for the other side: both sides launch the same seven kernels) runs 20
multi calls, or 20 loops, at Q = 8 and nothing else.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEQS, Q_PART, N_PARAS, N_ANSWERS = 5, 12, 5000, 8
PER_STEP = 8


def make_question(g, vocab, dev):
    """one net_input as the sampler collates it, on the device"""
    lens = torch.randint(200, 513, (SEQS,), generator=g)
    S = int(lens.max())
    ar = torch.arange(S)[None]
    mask = ar < lens[:, None]
    ids = torch.randint(1000, vocab, (SEQS, S), generator=g) * mask
    start = torch.full((SEQS, N_ANSWERS), -1)
    end = torch.full((SEQS, N_ANSWERS), -1)
    for b in range(SEQS):
        n = int(torch.randint(0, 4, (1,), generator=g))
        for a in range(n):
            s = int(torch.randint(Q_PART, int(lens[b]) - 6, (1,), generator=g))
            start[b, a], end[b, a] = s, s + int(torch.randint(0, 4, (1,), generator=g))
    start[0, 0], end[0, 0] = Q_PART + 3, Q_PART + 5
    labels = torch.zeros(N_PARAS, dtype=torch.int32)
    labels[torch.randint(0, N_PARAS, (6,), generator=g)] = 1
    idq = torch.randint(1000, vocab, (1, Q_PART), generator=g).expand(SEQS, Q_PART).contiguous()
    x = {"input_ids": ids, "input_mask": mask, "segment_ids": ((ar >= Q_PART) & mask).long(),
         "paragraph_mask": (ar >= Q_PART) & (ar < lens[:, None] - 1), "input_ids_q": idq, "input_mask_q": torch.ones_like(idq),
         "para_embed": (0.4 * torch.randn(N_PARAS, 128, generator=g)).half(), "top5000_labels": labels,
         "start_positions": start, "end_positions": end}
    return {k: v.to(dev) for k, v in x.items()}, [int(n) for n in lens]


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()


def take_turns(contenders, warmup, repeats):
    """{name: median milliseconds}; the contenders run one after the other inside every iteration"""
    events = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
              for name in contenders}
    for it in range(warmup + repeats):
        for name, fn in contenders.items():
            if it < warmup:
                fn()
            else:
                timed(fn, *events[name][it - warmup])
    torch.cuda.synchronize()
    return {name: statistics.median(a.elapsed_time(b) for a, b in ev) for name, ev in events.items()}


def loss_operands(questions, hidden_size, dev, g):
    """the operands of the loss for a pack of questions: random hidden states, the questions' geometry"""
    from proqa_amd.trainable_reader import _paragraph_geometry
    per = []
    for x, lens in questions:
        lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
        po, _ = _paragraph_geometry(x["paragraph_mask"], lens_t)
        cu = torch.zeros(SEQS + 1, dtype=torch.int32, device=dev)
        cu[1:] = torch.cumsum(lens_t, 0)
        hidden = torch.randn(sum(lens), hidden_size, generator=g).half().to(dev)
        per.append(dict(hidden=hidden, cu=cu, po=po, x=x, q=(0.4 * torch.randn(128, generator=g)).half().to(dev), lens=lens))
    return per


def loss_contenders(per, w, b):
    from proqa_amd.reader_loss import reader_loss, reader_loss_multi
    n = len(per)
    hidden = torch.cat([p["hidden"] for p in per]).requires_grad_(True)
    singles = [p["hidden"].clone().requires_grad_(True) for p in per]
    lens = torch.tensor([m for p in per for m in p["lens"]], dtype=torch.int32, device=hidden.device)
    cu = torch.zeros(lens.numel() + 1, dtype=torch.int32, device=hidden.device)
    cu[1:] = torch.cumsum(lens, 0)
    cat = lambda k: torch.cat([p["x"][k] for p in per])
    multi_args = dict(para_embed=cat("para_embed"), top5000_labels=cat("top5000_labels"), start_positions=cat("start_positions"),
                      end_positions=cat("end_positions"), para_offset=torch.cat([p["po"] for p in per]), cu_seqlens=cu,
                      question_seq=[SEQS * i for i in range(n + 1)], question_para=[N_PARAS * i for i in range(n + 1)],
                      max_seq_len=512)
    q = torch.stack([p["q"] for p in per]).requires_grad_(True)
    qs = [p["q"].clone().requires_grad_(True) for p in per]

    def multi():
        reader_loss_multi(hidden, w, b, q, **multi_args)["losses"].sum().backward()

    def loop():
        for p, h, qi in zip(per, singles, qs):
            x = p["x"]
            reader_loss(h, w, b, qi, x["para_embed"], x["top5000_labels"], x["start_positions"], x["end_positions"], p["po"],
                        cu_seqlens=p["cu"], max_seq_len=512)["loss"].backward()
    return {"multi": multi, "loop": loop}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--only-loss", type=int, default=0, help="Q: 20 calls of --route and nothing else (for a kernel trace)")
    ap.add_argument("--route", choices=("multi", "loop"), default="multi")
    ap.add_argument("--skip-pass", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from proqa_amd.optim import FusedAdamW
    from proqa_amd.reader import random_state_dict
    from proqa_amd.retriever import BERT_BASE
    from proqa_amd.trainable_reader import TrainableReader
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(21)
    questions = [make_question(g, BERT_BASE["vocab_size"], dev) for _ in range(16)]
    H = BERT_BASE["hidden_size"]
    w = (0.02 * torch.randn(2, H, generator=g)).to(dev).requires_grad_(True)
    b = torch.zeros(2, device=dev).requires_grad_(True)
    per = loss_operands(questions, H, dev, g)
    if args.only_loss:
        c = loss_contenders(per[:args.only_loss], w, b)
        for _ in range(20):
            c[args.route]()
        torch.cuda.synchronize()
        return
    result = {"shape": {"sequences": SEQS, "tokens": "200-512", "paras": N_PARAS, "answers": N_ANSWERS, "model": "bert-base"},
              "warmup": args.warmup, "repeats": args.repeats, "loss_ms": {}, "pass": {}}
    for n in (1, 4, 8, 16):
        ms = take_turns(loss_contenders(per[:n], w, b), args.warmup, args.repeats)
        result["loss_ms"][str(n)] = {"multi": ms["multi"], "loop": ms["loop"], "loop_over_multi": ms["loop"] / ms["multi"]}
        print("loss", n, result["loss_ms"][str(n)], flush=True)
    if not args.skip_pass:
        model = TrainableReader(BERT_BASE, dev, shared_norm=True)
        model.load_state_dict(random_state_dict(BERT_BASE, seed=0))
        model.train()
        opt = FusedAdamW([p for p in model.parameters()], lr=1e-5, max_grad_norm=5.0, loss_scale="dynamic")
        inputs = [x for x, _ in questions[:PER_STEP]]

        def step_of(size):
            def run():
                for at in range(0, PER_STEP, size):
                    if size == 1:
                        loss = model(inputs[at])["loss"] / PER_STEP
                    else:
                        loss = model(inputs[at:at + size])["losses"].sum() / PER_STEP
                    opt.scale_loss(loss).backward()
                opt.step()
                model.zero_grad()
            return run
        ms = take_turns({"dict": step_of(1), "list4": step_of(4), "list8": step_of(8), "dict_again": step_of(1),
                         "dict_third": step_of(1)}, args.warmup, args.repeats)
        qps = {k: PER_STEP * 1000.0 / v for k, v in ms.items()}
        ones = [qps["dict"], qps["dict_again"], qps["dict_third"]]
        result["pass"] = {"ms_per_8_questions": ms, "questions_per_second": qps, "dict_spread": max(ones) - min(ones),
                          "list8_over_dict": qps["list8"] / statistics.median(ones),
                          "list4_over_dict": qps["list4"] / statistics.median(ones)}
        print("pass", result["pass"], flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
