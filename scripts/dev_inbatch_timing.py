"""Kernel-only time of proqa_inbatch_eval_f16 (dev): the reference's operating point, batch 100 x 100, and a ClusterSampler-
sized 4096 x 4096.

    python scripts/dev_inbatch_timing.py [--out DIR] [--shapes 100x100,4096x4096] [--reps 50]

starts `rocprofv3 --kernel-trace` over a fresh child process of this script (--child: nothing but the launches; a run of
its own, no counters, no other tracing) and reads the kernel trace: per shape the median and minimum duration of
inbatch_eval (+ inbatch_combine where the columns are split), next to the flops (2 nq nc 128) and the compulsory bytes
((nq + nc) 256 in, 20 nq out) the shape implies, and the passage bytes the workgroups request from L2 (every 32-row
query tile reads every passage row once).  Prints one JSON line.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP = 5


def n_split(nq, nc):
    """The column split proqa_inbatch_eval_f16 takes (csrc/inbatch_kernels.hip): which shapes launch inbatch_combine."""
    q_tiles, c_tiles = -(-nq // 32), -(-nc // 32)
    if q_tiles >= 512:
        return 1
    s = max(1, min(-(-512 // q_tiles), -(-c_tiles // 16), 1024 // q_tiles))
    return -(-c_tiles // -(-c_tiles // s))


def child(shapes, reps):
    sys.path.insert(0, ROOT)
    import torch
    from proqa_amd.inbatch import inbatch_eval
    dev = torch.device("cuda", 0)
    for nq, nc in shapes:
        g = torch.Generator().manual_seed(nq * 7 + nc)
        q = torch.randn((nq, 128), generator=g).half().to(dev)
        c = torch.randn((nc, 128), generator=g).half().to(dev)
        for _ in range(WARMUP + reps):
            out = inbatch_eval(q, c)
        torch.cuda.synchronize()
        print(f"{nq}x{nc}: argmax[0]={int(out['argmax'][0])} lse[0]={float(out['lse'][0]):.4f}", file=sys.stderr)


def read_trace(out_dir):
    """[(kernel name, start ns, end ns)] of the run's kernel trace, in start order."""
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort(key=lambda r: r[1])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None, help="directory of the profiler's output (default: a temporary one)")
    ap.add_argument("--shapes", default="100x100,4096x4096")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.child:
        return child(shapes, args.reps)
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if args.out is None:
        import tempfile
        args.out = tempfile.mkdtemp(prefix="inbatch_timing_")
    os.makedirs(args.out, exist_ok=True)
    cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", args.out, "--", sys.executable, os.path.abspath(__file__),
           "--child", "--shapes", args.shapes, "--reps", str(args.reps)]
    subprocess.run(cmd, check=True, timeout=600)
    trace = read_trace(args.out)
    evals = [e - s for name, s, e in trace if "inbatch_eval" in name]
    combines = [e - s for name, s, e in trace if "inbatch_combine" in name]
    per = WARMUP + args.reps
    if len(evals) != per * len(shapes):
        raise SystemExit(f"expected {per * len(shapes)} inbatch_eval launches in the trace, found {len(evals)}")
    result = {"reps": args.reps, "shapes": []}
    k = 0
    for i, (nq, nc) in enumerate(shapes):
        ev = evals[i * per + WARMUP:(i + 1) * per]
        split = n_split(nq, nc)
        cb = []
        if split > 1:
            cb = combines[k * per + WARMUP:(k + 1) * per]
            k += 1
        total = [a + (b if cb else 0) for a, b in zip(ev, cb or ev)]
        us = statistics.median(total) / 1e3
        flops = 2.0 * nq * nc * 128
        io_bytes = (nq + nc) * 256 + 20 * nq
        l2_bytes = -(-nq // 32) * nc * 256
        result["shapes"].append({
            "nq": nq, "nc": nc, "n_split": split, "eval_us_median": statistics.median(ev) / 1e3, "eval_us_min": min(ev) / 1e3,
            "combine_us_median": statistics.median(cb) / 1e3 if cb else 0.0, "kernels_us_median": us,
            "flops": flops, "compulsory_bytes": io_bytes, "l2_request_bytes": l2_bytes,
            "tflops": flops / us / 1e6, "compulsory_gbs": io_bytes / us / 1e3, "l2_request_gbs": l2_bytes / us / 1e3})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
