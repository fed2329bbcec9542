"""Time of the embedding + LayerNorm backward with the word-embedding gradient summed by atomics (the default) and in a fixed
order (the *_det entry points) (dev).

    python scripts/dev_embed_word_grad_timing.py [--out DIR] [--json FILE] [--skip-trace]

The entry points are called directly over preallocated outputs (they are ADDED INTO: nothing is zeroed between launches, so
the dense torch.zeros(word.shape) of the Python wrapper is not part of the figure).  Two measurements, each in a fresh child
process of this script:
  events   the two routes take turns in one process; a launch between device events, median of 50 after 5 warm-ups;
  trace    `rocprofv3 --kernel-trace` (a run of its own: no counters, no other tracing): time per kernel name and launch.
Shapes, vocabulary 30522, hidden 768, seeded:
  retriever  80 sequences of lengths ~U[32, 128], Zipf-distributed ids, [CLS] first and [SEP] last in every sequence;
  reader     5 sequences of 200-512 tokens, typed, the same ids;
  one_id     the retriever's shape with every token of one id (the longest chain of partials).
Prints one JSON line (and writes it to --json).
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
WARMUP, LAUNCHES = 5, 50
VOCAB, HIDDEN, CLS, SEP = 30522, 768, 101, 102
SHAPES = ("retriever", "reader", "one_id")
KERNELS = ("embed_layernorm_typed_bwd_no_word", "embed_layernorm_bwd_no_word", "embed_layernorm_typed_bwd", "embed_layernorm_bwd",
           "reduce_slabs", "word_grad_keys", "word_grad_sort_pass", "word_grad_scan", "word_grad_units", "word_grad_combine")


def make_case(shape, dev):
    import torch
    g = torch.Generator().manual_seed(SHAPES.index(shape))
    typed = shape == "reader"
    lens = torch.randint(200, 513, (5,), generator=g) if typed else torch.randint(32, 129, (80,), generator=g)
    B, S, T = len(lens), int(lens.max()), int(lens.sum())
    # Zipf: rank r with probability ~ 1 / r over the word pieces 1000 ..
    ranks = torch.exp(torch.rand((B, S), generator=g, dtype=torch.float64) * torch.log(torch.tensor(float(VOCAB - 1000)))).long()
    ids = (999 + ranks).clamp_(max=VOCAB - 1)
    ids[:, 0] = CLS
    for b, n in enumerate(lens.tolist()):
        ids[b, n - 1] = SEP
    if shape == "one_id":
        ids[:] = 2000
    half = lambda *s: torch.randn(*s, generator=g).half().to(dev)
    type_ids = (torch.arange(S)[None] >= (lens[:, None] // 8)).long()
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    return dict(typed=typed, batch=B, seq_len=S, n_tokens=T, dy=half(T, HIDDEN), ids=ids.to(dev), type_ids=type_ids.to(dev),
                cu=cu.to(dev), word=half(VOCAB, HIDDEN), pos=half(512, HIDDEN), types=half(2, HIDDEN),
                gamma=(1.0 + 0.1 * torch.randn(HIDDEN, generator=g)).half().to(dev))


def launcher(c, deterministic, dev):
    """-> a function that launches the entry point once over buffers of its own"""
    import torch
    from proqa_amd import _lib
    lib = _lib.load()
    typed, T = c["typed"], c["n_tokens"]
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    out = dict(dgamma=f32(HIDDEN), dbeta=f32(HIDDEN), d_word=f32(VOCAB, HIDDEN), d_pos=f32(512, HIDDEN),
               d_types=f32(2, HIDDEN) if typed else f32(HIDDEN))
    if deterministic:
        need = lib.proqa_embed_layernorm_backward_det_workspace_bytes(T, HIDDEN, int(typed))
    else:
        need = lib.proqa_embed_layernorm_typed_backward_workspace_bytes(HIDDEN) if typed else lib.proqa_backward_workspace_bytes(HIDDEN)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    name = "proqa_embed_layernorm_" + ("typed_" if typed else "") + "varlen_backward_" + ("det_" if deterministic else "") + "f16"
    head = (c["dy"].data_ptr(), c["ids"].data_ptr()) + ((c["type_ids"].data_ptr(),) if typed else ())
    table = (c["types"].data_ptr(), 2) if typed else (c["types"].data_ptr(),)
    args = head + (c["cu"].data_ptr(), c["batch"], c["seq_len"], HIDDEN, T, c["word"].data_ptr(), VOCAB, c["pos"].data_ptr()) + table \
        + (c["gamma"].data_ptr(), 1e-12, out["dgamma"].data_ptr(), out["dbeta"].data_ptr(), out["d_word"].data_ptr(),
           out["d_pos"].data_ptr(), out["d_types"].data_ptr(), ws.data_ptr(), need, _lib.current_stream_ptr())
    fn = getattr(lib, name)

    def launch():
        status = fn(*args)
        if status != 0:
            raise RuntimeError(f"{name}: {status} {lib.proqa_last_error()}")
    launch.keep = (out, ws)
    return launch


def child():
    sys.path.insert(0, ROOT)
    import torch
    dev = torch.device("cuda", 0)
    result = {}
    with torch.cuda.device(dev):
        for shape in SHAPES:
            c = make_case(shape, dev)
            routes = {"atomic": launcher(c, False, dev), "deterministic": launcher(c, True, dev)}
            times = {k: [] for k in routes}
            for _ in range(WARMUP + LAUNCHES):
                for k, launch in routes.items():        # the routes take turns
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    launch()
                    t1.record()
                    torch.cuda.synchronize()
                    times[k].append(t0.elapsed_time(t1) * 1e3)
            med = {k: statistics.median(v[WARMUP:]) for k, v in times.items()}
            result[shape] = {"tokens": c["n_tokens"], "sequences": c["batch"], "typed": c["typed"],
                             "distinct_ids": int(c["ids"].unique().numel()),
                             **{f"{k}_us_median": v for k, v in med.items()}, **{f"{k}_us_min": min(v[WARMUP:]) for k, v in times.items()},
                             "deterministic_over_atomic": med["deterministic"] / med["atomic"]}
    print("RESULT " + json.dumps(result))


def run_child(prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child"]
    out = subprocess.run(cmd, check=True, timeout=600, capture_output=True, text=True).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def kernel_times(out_dir):
    """{shape: {route: {kernel: us per launch of the entry point}}}: the traced child launches, per shape, atomic and
    deterministic in turns -- a deterministic launch is told by its *_no_word kernel, and the trace is cut at each one of the
    two position kernels"""
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                tag = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
                if tag is not None:
                    rows.append((int(r["Start_Timestamp"]), tag, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    launches, current = [], None
    for _, tag, ns in rows:
        if tag.startswith("embed_layernorm"):
            current = {"route": "deterministic" if tag.endswith("no_word") else "atomic", "kernels": {}}
            launches.append(current)
        if current is not None:
            current["kernels"][tag] = current["kernels"].get(tag, 0) + ns
    per_shape = 2 * (WARMUP + LAUNCHES)
    result = {}
    for i, shape in enumerate(SHAPES):
        mine = launches[i * per_shape:(i + 1) * per_shape]
        result[shape] = {}
        for route in ("atomic", "deterministic"):
            runs = [l["kernels"] for l in mine if l["route"] == route][WARMUP:]
            names = sorted({k for r in runs for k in r})
            table = {k: statistics.median(r.get(k, 0) for r in runs) / 1e3 for k in names}
            table["total"] = statistics.median(sum(r.values()) for r in runs) / 1e3
            result[shape][route] = table
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-trace", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    sys.path.insert(0, ROOT)
    from proqa_amd import _lib
    result = {"rocm": open("/opt/rocm/.info/version").read().strip() if os.path.exists("/opt/rocm/.info/version") else "",
              "chunk": _lib.load().proqa_embed_word_grad_chunk(), "warmup": WARMUP, "launches": LAUNCHES, "events": run_child()}
    if not args.skip_trace:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if args.out is None:
            import tempfile
            args.out = tempfile.mkdtemp(prefix="word_grad_timing_")
        os.makedirs(args.out, exist_ok=True)
        run_child(prefix=[prof, "--kernel-trace", "--output-format", "csv", "-d", args.out, "--"])
        result["kernel_us_per_launch"] = kernel_times(args.out)
    line = json.dumps(result)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
