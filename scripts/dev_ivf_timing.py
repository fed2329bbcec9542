"""IndexIVFFlat at the reader's operating point, on seeded synthetic data (developer tool).

18M x 128 fp16 rows drawn around 4096 random centres (so that k-means finds uneven lists, as on real embeddings), nlist
100, nprobe 20 (qa/online_sampler.py:75-79), 2032 questions drawn the same way.  Prints one JSON line: train and add
time, search time for 2032 queries and for one query at k = 5 and k = 80 (median of --reps, host clock around a
synchronised call), rows scanned per query, the scan kernel's HIP-event time and its algorithmic rate 2 x 128 x (rows
scanned) / time as a fraction of the fp16 peak, and IndexFlatIP over the same rows and queries beside it.
`rocprofv3 --kernel-trace --stats -- python scripts/dev_ivf_timing.py --trace` in a run of its own gives the kernel
times of the searches alone (no flat index, one repetition each).

    python scripts/dev_ivf_timing.py [--rows 18000000] [--questions 2032] [--reps 10] [--peak-tflops 2500] [--trace]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic(n, centres, gen, dev, spread=0.6):
    lab = torch.randint(0, centres.shape[0], (n,), generator=gen, device=dev)
    out = torch.empty((n, 128), dtype=torch.float16, device=dev)
    step = 1 << 22
    for r0 in range(0, n, step):
        m = min(step, n - r0)
        noise = torch.randn((m, 128), generator=gen, device=dev)
        out[r0:r0 + m] = (centres[lab[r0:r0 + m]] + spread * noise).half()
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=18_000_000)
    ap.add_argument("--questions", type=int, default=2032)
    ap.add_argument("--nlist", type=int, default=100)
    ap.add_argument("--nprobe", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--peak-tflops", type=float, default=2500.0, help="dense fp16 peak of the device (MI355X: ~2.5 PFLOP/s)")
    ap.add_argument("--trace", action="store_true", help="searches only, one repetition each (for rocprofv3)")
    args = ap.parse_args()
    from proqa_amd.index import IndexFlatIP, IndexIVFFlat
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2032)
    centres = torch.randn((4096, 128), generator=gen, device=dev)
    x = synthetic(args.rows, centres, gen, dev)
    xq = synthetic(args.questions, centres, gen, dev)
    out = {"rows": args.rows, "questions": args.questions, "nlist": args.nlist, "nprobe": args.nprobe}

    index = IndexIVFFlat(IndexFlatIP(128), 128, args.nlist)
    torch.cuda.synchronize()
    t = time.perf_counter()
    index.train(x)
    torch.cuda.synchronize()
    out["train_s"] = round(time.perf_counter() - t, 3)
    t = time.perf_counter()
    index.add(x)
    torch.cuda.synchronize()
    out["add_s"] = round(time.perf_counter() - t, 3)
    index.nprobe = args.nprobe
    sizes = index.list_sizes()
    out["list_rows_min_median_max"] = [int(sizes.min()), int(statistics.median(sizes.tolist())), int(sizes.max())]
    reps = 1 if args.trace else args.reps
    for nq, tag in ((args.questions, "batch"), (1, "one")):
        for k in (5, 80):
            q = xq[:nq]
            index.search_device(q, k)                       # warm-up: workspace
            ms = timed(lambda: index.search_device(q, k), reps)
            st = index.last_stats()
            out[f"ivf_{tag}_k{k}_ms"] = round(ms, 3)
            out[f"ivf_{tag}_k{k}_scan_ms"] = round(st["scan_ms"], 3)
            out[f"ivf_{tag}_k{k}_work_items"] = st["work_items"]
            flops = 2.0 * 128 * st["rows_scanned"]
            out[f"ivf_{tag}_k{k}_scan_peak_fraction"] = round(flops / (st["scan_ms"] * 1e-3) / (args.peak_tflops * 1e12), 4)
            if tag == "batch" and k == 5:
                out["rows_scanned_per_query"] = round(st["rows_scanned_per_query"])
                out["scan_tflop"] = round(flops / 1e12, 3)
    if not args.trace:
        del index
        flat = IndexFlatIP(128)
        flat.adopt_device(x)
        flat.prepare()
        for nq, tag in ((args.questions, "batch"), (1, "one")):
            for k in (5, 80):
                q = xq[:nq]
                flat.search_device(q, k)
                out[f"flat_{tag}_k{k}_ms"] = round(timed(lambda: flat.search_device(q, k), args.reps), 3)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
