"""Time of the weight-gradient product dw[N, K] = dy^T x (dev): proqa_linear_wgrad_f16 against the pair it replaced in
proqa_amd.trainable, `dy.t() @ x` in fp16 (rocBLAS / hipBLASLt) followed by `.float()`.

    python scripts/dev_wgrad_timing.py [--out DIR] [--tokens 81920,8192] [--launches 50] [--skip-trace]

Shapes: the four weight shapes of bert-base, (N, K) = (2304, 768) (Q|K|V), (768, 768), (3072, 768), (768, 3072), at
T = 81 920 (640 paragraphs of 128 tokens) and T = 8 192.  Two measurements, each in a fresh child process of this script:
  events   the contenders take turns in one process; one launch between two device events, median of --launches after 5
           warm-ups; the fraction of the 2.5 PFLOP/s fp16 dense peak by 2 T N K, and the ratio to the replaced pair;
  trace    `rocprofv3 --kernel-trace` (a run of its own: no counters, no other tracing) over the same launches: device time
           per launch of our two kernels and of the library's kernels (the GEMM and the cast).
Prints one JSON line.
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
PEAK_TFLOPS = 2500.0      # fp16 dense, MI355X
SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]


def child(tokens, launches):
    sys.path.insert(0, ROOT)
    import torch
    from proqa_amd.trainable import linear_wgrad
    dev = torch.device("cuda", 0)
    result = {}
    for T in tokens:
        for N, K in SHAPES:
            g = torch.Generator().manual_seed(T + N + K)
            dy = torch.randn((T, N), generator=g).half().to(dev)
            x = torch.randn((T, K), generator=g).half().to(dev)
            out = torch.empty((N, K), dtype=torch.float32, device=dev)
            contenders = {"wgrad_kernel": lambda: linear_wgrad(dy, x, out=out),
                          "fp16_gemm_then_cast": lambda: (dy.t() @ x).float()}
            times = {k: [] for k in contenders}
            for i in range(WARMUP + launches):
                for name, fn in contenders.items():      # taking turns: both see the same clocks and the same neighbours
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    fn()
                    t1.record()
                    torch.cuda.synchronize()
                    if i >= WARMUP:
                        times[name].append(t0.elapsed_time(t1) * 1e3)
            err = ((dy.t() @ x).float() - out).abs().max().item() / out.abs().max().item()
            us = {k: statistics.median(v) for k, v in times.items()}
            result[f"T={T} N={N} K={K}"] = {
                "us_median": us, "us_min": {k: min(v) for k, v in times.items()},
                "fraction_of_fp16_peak": {k: 2.0 * T * N * K / (v * 1e-6) / 1e12 / PEAK_TFLOPS for k, v in us.items()},
                "kernel_over_replaced": us["wgrad_kernel"] / us["fp16_gemm_then_cast"],
                "fp16_path_differs_by": err}
    print("RESULT " + json.dumps(result))


def run_child(args, tokens, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", "--tokens", tokens, "--launches", str(args.launches)]
    out = subprocess.run(cmd, check=True, timeout=900, capture_output=True, text=True).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def short(name):
    for tag in ("wgrad_tile_kernel", "wgrad_reduce"):
        if tag in name:
            return tag
    return "gemm (library)" if ("Cijk" in name or "gemm" in name.lower()) else "torch: " + name.split("(")[0][-60:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", default="81920,8192")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--skip-trace", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child([int(t) for t in args.tokens.split(",")], args.launches)
    result = {"events": run_child(args, args.tokens)}
    if not args.skip_trace:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if args.out is None:
            import tempfile
            args.out = tempfile.mkdtemp(prefix="wgrad_timing_")
        result["trace_us_per_launch"] = {}
        for T in args.tokens.split(","):      # one traced run per token count; the four shapes share it, told apart by order
            d = os.path.join(args.out, T)
            os.makedirs(d, exist_ok=True)
            run_child(args, T, prefix=[prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
            rows = []
            for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                with open(path, newline="") as f:
                    rows += [(int(r["Start_Timestamp"]), short(r["Kernel_Name"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                             for r in csv.DictReader(f)]
            rows.sort()
            # the launches of a shape are contiguous in time: cut the trace at every (WARMUP + launches)-th tile kernel
            per_shape, seen = [{} for _ in SHAPES], 0
            for _, name, ns in rows:
                if name == "wgrad_tile_kernel":
                    seen += 1
                if name.startswith("torch: ") and "float" not in name.lower() and "copy" not in name.lower():
                    continue                   # (the error check's reductions, not a contender)
                idx = min(max(seen - 1, 0) // (WARMUP + args.launches), len(SHAPES) - 1)
                total, count = per_shape[idx].get(name, (0, 0))
                per_shape[idx][name] = (total + ns, count + 1)
            for (N, K), per in zip(SHAPES, per_shape):      # mean device time of one launch of each kernel
                result["trace_us_per_launch"][f"T={T} N={N} K={K}"] = {k: v / c / 1e3 for k, (v, c) in sorted(per.items())}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
