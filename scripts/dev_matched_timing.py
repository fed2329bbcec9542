"""The matched-paragraph command on a seeded synthetic corpus: device pre-filter against host pre-filter (developer tool).

--docs passages of 100 words (a 20 000-word vocabulary, ~650 bytes each; 1 M passages = 650 MB of text, past the Infinity
Cache) with random 128-d fp16 embeddings, an .ids id map and a text sidecar generated in bulk (as bench.py's CLI legs do);
--questions questions whose answers are two consecutive words of a random passage and one random word of the vocabulary;
k = --k.  process_ground_paras runs with prefilter="device", then with prefilter="host", in one process; both files must be
equal.  With --trace the device route runs once more as a child under `rocprofv3 --kernel-trace`, and the launches of
text_prefilter are summed: the kernel's own time, and its rate over candidates x mean folded text bytes (nominal: a passage
is left as soon as one alias is complete) against the 8 TB/s of the HBM.

    python scripts/dev_matched_timing.py [--docs 1000000] [--questions 2032] [--k 10000] [--workers 16] [--trace]
                                         [--dir DIR] [--out profiles/rNN_matched_timing.json]

Prints one JSON line: seconds per stage of both routes, candidates, survivors, confirmed, the survivor fraction, and with
--trace the kernel's milliseconds and TB/s.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VOCAB, WORDS_PER_DOC = 20000, 100


def make_corpus(d, docs, questions, seed=3):
    """para_embed.npy, query.npy, qa.txt, idx_id.ids (+ .off.npy) and the text sidecar idx_id.txt (+ .txtoff.npy) under d"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    vocab = [bytes(rng.choice(letters, size=int(rng.integers(3, 10))).tolist()) for _ in range(VOCAB)]
    vocab_s = np.asarray([w + b" " for w in vocab], dtype="S10")
    word_len = np.asarray([len(w) + 1 for w in vocab], np.int64)
    spans = np.zeros((docs, 2), np.int64)
    pos = 0
    keep = {}                                  # the word rows of the passages the answers are cut from
    answer_docs = rng.integers(0, docs, questions)
    with open(os.path.join(d, "idx_id.txt"), "wb") as f:
        for d0 in range(0, docs, 100_000):
            idx = rng.integers(0, VOCAB, (min(100_000, docs - d0), WORDS_PER_DOC))
            lens = word_len[idx].sum(1)
            ends = pos + np.cumsum(lens)
            spans[d0:d0 + len(idx)] = np.stack([ends - lens, ends], axis=1)
            f.write(vocab_s[idx].tobytes().replace(b"\0", b""))
            pos = int(ends[-1])
            for q in np.nonzero((answer_docs >= d0) & (answer_docs < d0 + len(idx)))[0]:
                keep[int(q)] = idx[answer_docs[q] - d0]
    np.save(os.path.join(d, "idx_id.txtoff.npy"), spans)
    ids = np.arange(docs, dtype=np.int64)
    blob = np.empty((docs, 11), dtype=np.uint8)
    blob[:, 0], blob[:, 1], blob[:, 9], blob[:, 10] = ord('"'), ord("d"), ord('"'), ord("\n")
    for j in range(7):
        blob[:, 8 - j] = ord("0") + (ids // 10 ** j) % 10
    blob.tofile(os.path.join(d, "idx_id.ids"))
    np.save(os.path.join(d, "idx_id.off.npy"), np.arange(docs + 1, dtype=np.int64) * 11)
    with open(os.path.join(d, "qa.txt"), "w") as f:
        for q in range(questions):
            p = int(rng.integers(0, WORDS_PER_DOC - 1))
            pair = (vocab[keep[q][p]] + b" " + vocab[keep[q][p + 1]]).decode().title()
            f.write(json.dumps({"question": f"question number {q}",
                                "answer": [pair, vocab[int(rng.integers(0, VOCAB))].decode()]}) + "\n")
    with open(os.path.join(d, "para_embed.npy"), "wb") as f:
        np.lib.format.write_array_header_1_0(f, {"descr": "<f2", "fortran_order": False, "shape": (docs, 128)})
        for d0 in range(0, docs, 200_000):
            f.write(rng.standard_normal((min(200_000, docs - d0), 128), dtype=np.float32).astype(np.float16).data)
    np.save(os.path.join(d, "query.npy"), rng.standard_normal((questions, 128), dtype=np.float32).astype(np.float16))
    return pos


def run_route(d, route, args):
    from proqa_amd import prepro_dense
    out = os.path.join(d, f"matched_{route}.txt")
    t0 = time.perf_counter()
    prepro_dense.process_ground_paras(None, out, os.path.join(d, "qa.txt"), args.workers, False, args.k, "string",
                                      index_path=os.path.join(d, "para_embed.npy"), query_embeds=os.path.join(d, "query.npy"),
                                      index2paraid=os.path.join(d, "idx_id.ids"), text_sidecar=os.path.join(d, "idx_id.txt"),
                                      prefilter=route)
    return dict(prepro_dense.LAST_RUN_STATS, wall_seconds=time.perf_counter() - t0), out


def trace(d, args, nominal_bytes):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out_dir = os.path.join(d, "trace")
    cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
           "--trace-child", "--dir", d, "--docs", str(args.docs), "--questions", str(args.questions), "--k", str(args.k),
           "--workers", str(args.workers)]
    subprocess.run(cmd, check=True, timeout=1000, stdout=subprocess.DEVNULL)
    ns = {"text_prefilter": [], "text_prefilter_count": []}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                if "text_prefilter" in name:
                    ns["text_prefilter_count" if "text_prefilter_count" in name else "text_prefilter"].append(
                        int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    if not ns["text_prefilter"]:
        raise RuntimeError("no text_prefilter launch in the kernel trace")
    ms = sum(ns["text_prefilter"]) / 1e6
    return {"launches": len(ns["text_prefilter"]), "text_prefilter_ms": ms, "text_prefilter_count_ms": sum(ns["text_prefilter_count"]) / 1e6,
            "nominal_text_bytes": int(nominal_bytes), "nominal_TBps": nominal_bytes / (ms / 1e3) / 1e12,
            "fraction_of_8TBps": nominal_bytes / (ms / 1e3) / 8e12}


ROUTE_STAGES = ("needles_seconds", "fold_seconds", "upload_seconds", "search_seconds", "prefilter_seconds", "confirm_seconds",
                "write_seconds")


def summarise(result):
    """The figures read off the two stats records.  route_seconds: the stages that belong to a route.  index_load_seconds
    is left out of it: the route that runs first in the process (the device route) pays PyTorch's start-up on the device
    there, the second one does not."""
    device, host = result["device"], result["host"]
    for st in (device, host):
        st["route_seconds"] = sum(st.get(key, 0.0) for key in ROUTE_STAGES)
    result.update(survivor_fraction=device["survivors"] / max(device["candidates"], 1),
                  host_over_device_route_seconds=host["route_seconds"] / device["route_seconds"],
                  host_over_device_wall=host["wall_seconds"] / device["wall_seconds"],
                  host_confirm_over_device_prefilter_plus_confirm=host["confirm_seconds"] / (
                      device["prefilter_seconds"] + device["confirm_seconds"]),
                  device_prefilter_over_search_seconds=device["prefilter_seconds"] / max(device["search_seconds"], 1e-9))
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--questions", type=int, default=2032)
    ap.add_argument("--k", type=int, default=10000)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--dir", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        run_route(args.dir, "device", args)
        return
    d = args.dir or tempfile.mkdtemp(prefix="proqa_matched_timing_")
    os.makedirs(d, exist_ok=True)
    try:
        t0 = time.perf_counter()
        text_bytes = make_corpus(d, args.docs, args.questions)
        result = {"docs": args.docs, "questions": args.questions, "k": args.k, "workers": args.workers, "text_bytes": text_bytes,
                  "corpus_seconds": time.perf_counter() - t0}
        device, dev_file = run_route(d, "device", args)
        host, host_file = run_route(d, "host", args)
        with open(dev_file, "rb") as a, open(host_file, "rb") as b:
            result["files_equal"] = a.read() == b.read()
        result.update(device=device, host=host)
        summarise(result)
        if args.trace:
            result["kernel_trace"] = trace(d, args, device["candidates"] * text_bytes / args.docs)
        line = json.dumps(result)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
    finally:
        if not args.dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
