"""Reader throughput at the reference's --do_predict operating point, on seeded synthetic data (developer tool).

2032 questions x eval_k 5 = 10160 sequences of [CLS] q [SEP] p [SEP], q 8-20 pieces, passages of 150-400 words
(~1.3 pieces per word, cut at max_seq_length 512), bert-base geometry with random fp16 weights, packed batches of
--batch sequences.  Prints one JSON line: reader sequences/s and tokens/s, the FP16 fraction of the dense peak from FLOPs
counted out of the shapes, and the span kernel's own time and GB/s over its T x hidden x 2 bytes (CUDA events around
repeated launches on the hidden states of one batch; `rocprofv3 --kernel-trace --stats` in a run of its own gives the
same kernel's trace).

    python scripts/dev_reader_timing.py [--questions 2032] [--k 5] [--batch 256] [--peak-tflops 2500]
    python scripts/dev_reader_timing.py --cli [--passages 20000]   # the whole --do_predict command, phase by phase
    python scripts/dev_reader_timing.py --cli --n-best 20          # the same with marginal decoding (postprocess_seconds)
    python scripts/dev_reader_timing.py --n-best 1,5,20            # the n-best span kernel against the 1-best one

--n-best without --cli: on the hidden states of one batch the 1-best kernel and the n-best kernel at every N of the list
take turns in one process, 5 warm-up rounds and --span-reps timed ones.  The kernel times are those of a
`rocprofv3 --kernel-trace` run of its own (this script starts it around a child of itself) and the figure is the median per
variant; the yardstick is the 1-best kernel of the same run.  Prints one JSON line with the medians and their ratios.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_pairs(n, max_len, seed=0, vocab=30522):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q = int(rng.integers(8, 21)) + 2
        p = min(int(rng.integers(150, 401) * 1.3), max_len - q - 1)
        L = q + p + 1
        ids = rng.integers(1000, vocab, L)
        ids[0], ids[q - 1], ids[L - 1] = 101, 102, 102
        seg = np.r_[np.zeros(q, np.int64), np.ones(L - q, np.int64)]
        out.append((ids, seg, q))
    return out


def run_cli(args):
    """The whole --do_predict command on a synthetic world: a bert-base-sized vocabulary of made-up words, random reader
    weights, --passages passages of 150-400 words in a sqlite DB with their random fp16 index rows, --questions questions.
    Prints the command's wall time split into search / pair building / reader / post-processing (PROQA_STATS_JSON)."""
    import sqlite3
    import tempfile
    from proqa_amd import predict_qa
    from proqa_amd.reader import random_state_dict
    from proqa_amd.retriever import BERT_BASE
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as tmp:
        special = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
        words = [f"w{i}" for i in range(BERT_BASE["vocab_size"] - len(special))]
        model_dir = os.path.join(tmp, "model")
        os.makedirs(model_dir)
        with open(os.path.join(model_dir, "vocab.txt"), "w") as f:
            f.write("\n".join(special + words) + "\n")
        with open(os.path.join(model_dir, "config.json"), "w") as f:
            json.dump(dict(BERT_BASE, model_type="bert"), f)
        torch.save({k: v.half() for k, v in random_state_dict(BERT_BASE, seed=0).items()}, os.path.join(tmp, "reader.pt"))
        warr = np.asarray(words)
        con = sqlite3.connect(os.path.join(tmp, "docs.db"))
        con.execute("CREATE TABLE documents (id PRIMARY KEY, text)")
        con.executemany("INSERT INTO documents VALUES (?, ?)",
                        ((f"d{p}", " ".join(warr[rng.integers(0, len(words), int(rng.integers(150, 401)))]))
                         for p in range(args.passages)))
        con.commit()
        con.close()
        np.save(os.path.join(tmp, "embed.npy"), rng.standard_normal((args.passages, 128)).astype(np.float16))
        with open(os.path.join(tmp, "idx_id.json"), "w") as f:
            json.dump({str(p): f"d{p}" for p in range(args.passages)}, f)
        with open(os.path.join(tmp, "qa.txt"), "w") as f:
            for _ in range(args.questions):
                q = " ".join(warr[rng.integers(0, len(words), int(rng.integers(5, 16)))])
                f.write(json.dumps({"question": q, "answer": [str(warr[rng.integers(0, len(words))])]}) + "\n")
        os.environ["PROQA_STATS_JSON"] = os.path.join(tmp, "stats.json")
        argv = ["--do_predict", "--raw-eval-data", f"{tmp}/qa.txt", "--init_checkpoint", f"{tmp}/reader.pt",
                "--index-path", f"{tmp}/embed.npy", "--db-path", f"{tmp}/docs.db", "--index2paraid", f"{tmp}/idx_id.json",
                "--eval-k", str(args.k), "--max_seq_length", str(args.max_seq_length), "--bert_model_name", model_dir,
                "--efficient_eval", "--reader-batch", str(args.batch)]
        if args.n_best:
            argv += ["--n-best", args.n_best]
        t0 = time.perf_counter()
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            predict_qa.main(argv)
        wall = time.perf_counter() - t0
        with open(os.environ["PROQA_STATS_JSON"]) as f:
            stats = json.load(f)
    print(json.dumps({"cli_wall_seconds": round(wall, 3), **{k: (round(v, 3) if isinstance(v, float) else v)
                                                              for k, v in stats.items()}}))


NBEST_WARMUP = 5


def first_batch(args, dev):
    """(reader, hidden states, seq_lens, para_offset, max_len) of the first --batch synthetic sequences"""
    from proqa_amd.reader import BertReader, random_state_dict
    from proqa_amd.retriever import BERT_BASE
    reader = BertReader.load(random_state_dict(BERT_BASE, seed=0), BERT_BASE, dev)
    chunk = synthetic_pairs(args.batch, args.max_seq_length)
    W = max(len(c[0]) for c in chunk)
    I = np.zeros((len(chunk), W), np.int64)
    S = np.zeros((len(chunk), W), np.int64)
    for k, (ids, seg, _) in enumerate(chunk):
        I[k, :len(ids)], S[k, :len(seg)] = ids, seg
    lens = [len(c[0]) for c in chunk]
    hid, _ = reader.hidden(torch.from_numpy(I).to(dev), torch.from_numpy(S).to(dev), lens)
    return reader, hid, lens, [c[2] for c in chunk], W


def nbest_child(args, ns):
    """the launches the trace is taken of: per round the 1-best kernel, then the n-best kernel at every N"""
    dev = torch.device("cuda:0")
    reader, hid, lens, po, W = first_batch(args, dev)
    for _ in range(NBEST_WARMUP + args.span_reps):
        reader.span(hid, lens, po, W)
        for n in ns:
            reader.span(hid, lens, po, W, n_best=n)
    torch.cuda.synchronize()
    print(json.dumps({"span_batch_tokens": int(hid.shape[0]), "sequences": len(lens)}))


def nbest_trace(args, ns):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out_dir = args.out
    if out_dir is None:
        import tempfile
        out_dir = tempfile.mkdtemp(prefix="reader_nbest_timing_")
    os.makedirs(out_dir, exist_ok=True)
    cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
           "--nbest-child", "--n-best", args.n_best, "--batch", str(args.batch), "--max-seq-length", str(args.max_seq_length),
           "--span-reps", str(args.span_reps)]
    child = subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.PIPE, text=True)
    launches = []           # (start, end, is n-best) of both span kernels, in time order
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "reader_span" in r["Kernel_Name"]:
                    launches.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "reader_span_nbest" in r["Kernel_Name"]))
    launches.sort()
    rounds, per = NBEST_WARMUP + args.span_reps, 1 + len(ns)
    if len(launches) != rounds * per:
        raise SystemExit(f"expected {rounds * per} span launches in the trace, found {len(launches)}")
    names = ["1-best"] + [f"n={n}" for n in ns]
    us = {}
    for k, name in enumerate(names):
        mine = launches[k::per]
        if any(l[2] != (k > 0) for l in mine):
            raise SystemExit("the trace's launches are not in the order they were issued")
        us[name] = statistics.median(e - s for s, e, _ in mine[NBEST_WARMUP:]) / 1e3
    result = json.loads(child.stdout.strip().splitlines()[-1])
    result.update(reps=args.span_reps, kernel_us_median={k: round(v, 2) for k, v in us.items()},
                  ratio_to_1best={k: round(v / us["1-best"], 3) for k, v in us.items() if k != "1-best"})
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cli", action="store_true", help="time the whole --do_predict command instead (synthetic world)")
    ap.add_argument("--passages", type=int, default=20000)
    ap.add_argument("--questions", type=int, default=2032)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--max-seq-length", type=int, default=512)
    ap.add_argument("--peak-tflops", type=float, default=2500.0, help="dense fp16 peak of the device (MI355X: ~2.5 PFLOP/s)")
    ap.add_argument("--span-reps", type=int, default=50)
    ap.add_argument("--n-best", type=str, default="",
                    help="with --cli: --n-best of the command; without: the Ns of the n-best kernel to time, e.g. 1,5,20")
    ap.add_argument("--nbest-child", action="store_true", help="(the traced child of --n-best)")
    ap.add_argument("--out", default=None, help="--n-best: directory of the profiler's output (default: a temporary one)")
    args = ap.parse_args()
    if args.cli:
        return run_cli(args)
    if args.n_best:
        ns = [int(n) for n in args.n_best.split(",")]
        return nbest_child(args, ns) if args.nbest_child else nbest_trace(args, ns)
    from proqa_amd.reader import BertReader, random_state_dict
    from proqa_amd.retriever import BERT_BASE
    dev = torch.device("cuda:0")
    reader = BertReader.load(random_state_dict(BERT_BASE, seed=0), BERT_BASE, dev)
    pairs = synthetic_pairs(args.questions * args.k, args.max_seq_length)
    batches = []
    for b0 in range(0, len(pairs), args.batch):
        chunk = pairs[b0:b0 + args.batch]
        W = max(len(c[0]) for c in chunk)
        I = np.zeros((len(chunk), W), np.int64)
        S = np.zeros((len(chunk), W), np.int64)
        for k, (ids, seg, _) in enumerate(chunk):
            I[k, :len(ids)], S[k, :len(seg)] = ids, seg
        batches.append({"input_ids": torch.from_numpy(I).to(dev), "segment_ids": torch.from_numpy(S).to(dev),
                        "seq_lens": [len(c[0]) for c in chunk], "para_offset": [c[2] for c in chunk]})
    reader.forward(batches[0])                       # workspace, library handles
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in batches:
        out = reader.forward(b)
    out["start"].cpu()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    tokens = sum(len(p[0]) for p in pairs)
    H, I_, NL = BERT_BASE["hidden_size"], BERT_BASE["intermediate_size"], BERT_BASE["num_hidden_layers"]
    dense = 2 * tokens * NL * (4 * H * H + 2 * H * I_)
    attn = sum(4 * len(p[0]) ** 2 * H for p in pairs) * NL
    flops = dense + attn

    # the span kernel alone, on one batch's hidden states
    b = batches[0]
    hid, _ = reader.hidden(b["input_ids"], b["segment_ids"], b["seq_lens"])
    reader.span(hid, b["seq_lens"], b["para_offset"], b["input_ids"].shape[1])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.span_reps):
        reader.span(hid, b["seq_lens"], b["para_offset"], b["input_ids"].shape[1])
    e1.record()
    e1.synchronize()
    span_ms = e0.elapsed_time(e1) / args.span_reps
    span_bytes = hid.shape[0] * H * 2
    print(json.dumps({
        "sequences": len(pairs), "tokens": tokens, "batch": args.batch, "reader_seconds": round(wall, 4),
        "sequences_per_s": round(len(pairs) / wall, 1), "tokens_per_s": round(tokens / wall, 1),
        "model_tflop": round(flops / 1e12, 2), "fp16_fraction_of_peak": round(flops / wall / 1e12 / args.peak_tflops, 3),
        "span_batch_tokens": int(hid.shape[0]), "span_ms_per_launch_incl_host": round(span_ms, 4),
        "span_gb_per_s": round(span_bytes / (span_ms * 1e-3) / 1e9, 1)}))


if __name__ == "__main__":
    main()
