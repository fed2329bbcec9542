"""What a trainer-state snapshot costs the training stream and the host (dev): proqa_amd.checkpoint against what a user had
to do before it for the same content, torch.save of the model's and the optimizer's state_dict from the device.

    python scripts/dev_checkpoint_timing.py [--out DIR] [--rounds 20] [--skip-trace] [--skip-events]

Tensors: the shapes of two bert-base towers and the two projections (proqa_amd.trainable._parameter_shapes: about 219 M
fp32 parameters), FusedAdamW over them, so that the state is 3 x 219 M fp32 words (masters, exp_avg, exp_avg_sq) in about
1 200 tensors.  Contenders, taking turns in one process, every call between device events on the training stream and host
clocks, median of --rounds after 3 warm-up rounds:
  torch_save   torch.save({"model": model.state_dict(), "optimizer": optimizer.state_dict()}, file)
  snapshot     StateSnapshotter.snapshot(file, meta): `held` is the call alone (the stream is busy for the one kernel, the
               host for the launch); `written_ms` is the time until the file is on disk (wait()), which training does not
               wait for
  copies       the yardstick of the kernel: dst[i].copy_(src[i]) over the same tensors, device to device
  foreach      the same through torch._foreach_copy_
`rocprofv3 --kernel-trace` (a run of its own): the kernel time of state_copy_digest (copy mode and digest only) and of the
kernels of one round of the device-to-device copies, and 8 bytes per element over the kernel time against
proqa_microbench_stream's copy rate on the same box.  Prints one JSON line.
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
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP = 3
TRACE_ROUNDS = 5


def make_state(dev):
    """(module, optimizer, StateSnapshotter over masters, both moments and the optimizer's scalars)"""
    import torch
    from proqa_amd import checkpoint
    from proqa_amd.optim import FusedAdamW
    from proqa_amd.retriever import BERT_BASE, config_from_dict
    from proqa_amd.trainable import _parameter_shapes
    gen = torch.Generator(device=dev).manual_seed(0)
    shapes = _parameter_shapes(config_from_dict(BERT_BASE))
    model = torch.nn.Module()
    model.weights = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=gen, device=dev) * 0.02)
                                            for s in shapes.values()])
    opt = FusedAdamW(list(model.parameters()), lr=1e-5, weight_decay=0.01, max_grad_norm=2.0, loss_scale="dynamic")
    for p in model.parameters():          # one step, so that the moments are not zeros
        p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-3
    opt.step()
    opt.zero_grad(set_to_none=True)
    names, tensors = checkpoint._named_state(model, opt)
    return model, opt, checkpoint.StateSnapshotter(tensors, names)


def child(mode, rounds, out_dir):
    sys.path.insert(0, ROOT)
    import torch
    dev = torch.device("cuda", 0)
    if mode == "stream":
        import ctypes
        from proqa_amd import _lib
        lib = _lib.load()
        nbytes = 2 << 30
        buf = torch.zeros(2 * nbytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        v = ctypes.c_double()
        _lib.check(lib.proqa_microbench_stream(buf.data_ptr(), nbytes, 0, 5, _lib.current_stream_ptr(), ctypes.byref(v)))
        print("RESULT " + json.dumps({"hbm_copy_GBs": v.value}))
        return
    model, opt, snap = make_state(dev)
    srcs = snap.tensors
    dsts = [torch.empty_like(t) for t in srcs]
    elements = int(sum(t.numel() for t in srcs))
    result = {"elements": elements, "tensors": len(srcs), "bytes_moved_by_the_kernel": 8 * elements}
    snap.prepare()
    torch.cuda.synchronize()
    if mode == "trace":
        for _ in range(TRACE_ROUNDS):
            snap._launch(True, snap._digests)
        for _ in range(TRACE_ROUNDS):
            snap.digest()
        for _ in range(TRACE_ROUNDS):
            for d, s in zip(dsts, srcs):
                d.copy_(s)
        torch.cuda.synchronize()
        print("RESULT " + json.dumps(result))
        return
    files = {n: os.path.join(out_dir, n + ".pt") for n in ("torch_save", "snapshot")}
    written = []

    def torch_save():
        torch.save({"model": model.state_dict(), "optimizer": opt.state_dict()}, files["torch_save"])

    def snapshot():
        snap.snapshot(files["snapshot"], {"global_step": 1})

    def copies():
        for d, s in zip(dsts, srcs):
            d.copy_(s)

    def foreach():
        torch._foreach_copy_(dsts, srcs)

    contenders = {"torch_save": torch_save, "snapshot": snapshot, "copies": copies, "foreach": foreach}
    held_ms = {n: [] for n in contenders}
    host_ms = {n: [] for n in contenders}
    for _ in range(WARMUP + rounds):
        for name, call in contenders.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            call()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if name == "snapshot":
                snap.wait()
                written.append((time.perf_counter() - t0) * 1e3)
            held_ms[name].append(e0.elapsed_time(e1))
            host_ms[name].append((t1 - t0) * 1e3)
    for name in contenders:
        d, h = held_ms[name][WARMUP:], host_ms[name][WARMUP:]
        result[name] = {"stream_held_ms_median": statistics.median(d), "stream_held_ms_min": min(d), "stream_held_ms_max": max(d),
                        "host_held_ms_median": statistics.median(h), "rounds": len(d)}
    result["snapshot"]["written_ms_median"] = statistics.median(written[WARMUP:])
    result["file_bytes"] = {n: os.path.getsize(p) for n, p in files.items()}
    snap.close()
    print("RESULT " + json.dumps(result))


def run_child(mode, rounds, out_dir, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", mode, "--rounds", str(rounds), "--out", out_dir]
    try:
        out = subprocess.run(cmd, check=True, timeout=1100, capture_output=True, text=True).stdout
    except subprocess.CalledProcessError as e:
        print((e.stderr or "")[-4000:], file=sys.stderr)
        raise
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def read_trace(out_dir):
    per = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                per.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, choices=["events", "trace", "stream"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--skip-events", action="store_true")
    args = ap.parse_args()
    if args.out is None:
        args.out = tempfile.mkdtemp(prefix="checkpoint_timing_")
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        return child(args.child, args.rounds, args.out)
    result = {"stream": run_child("stream", args.rounds, args.out)}
    if not args.skip_events:
        result["events"] = run_child("events", args.rounds, args.out)
    for name in ("torch_save.pt", "snapshot.pt"):          # 2.6 GB each: not left behind
        if os.path.exists(os.path.join(args.out, name)):
            os.remove(os.path.join(args.out, name))
    if not args.skip_trace:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        d = os.path.join(args.out, "trace")
        os.makedirs(d, exist_ok=True)
        info = run_child("trace", args.rounds, args.out, prefix=[prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
        per = read_trace(d)
        trace = {}
        for tags, key in ((("state_copy_digest<true>", "state_copy_digestILb1"), "copy_digest"),
                          (("state_copy_digest<false>", "state_copy_digestILb0"), "digest_only"),
                          (("state_digest_finish",), "finish")):
            times = [t for k, v in per.items() if any(tag in k for tag in tags) for t in v]
            trace[key + "_us_median"] = statistics.median(times) / 1e3 if times else None
            trace[key + "_launches"] = len(times)
        # what a device-to-device copy_ of a contiguous tensor launches: the runtime's buffer copy (or torch's copy kernel)
        copy_kernels = {k: v for k, v in per.items() if "copyBuffer" in k or "direct_copy" in k or "CopyFunctor" in k}
        trace["copies_us_per_round"] = sum(sum(v) for v in copy_kernels.values()) / TRACE_ROUNDS / 1e3
        trace["copies_launches_per_round"] = sum(len(v) for v in copy_kernels.values()) / TRACE_ROUNDS
        trace["copies_kernel_names"] = sorted(copy_kernels)[:8]
        if trace["copy_digest_us_median"]:
            gbs = info["bytes_moved_by_the_kernel"] / (trace["copy_digest_us_median"] * 1e-6) / 1e9
            trace["copy_digest_GBs"] = gbs
            trace["fraction_of_measured_copy_rate"] = gbs / result["stream"]["hbm_copy_GBs"]
            trace["kernel_over_copies"] = trace["copy_digest_us_median"] / trace["copies_us_per_round"] if trace["copies_us_per_round"] else None
        result["trace"] = trace
    print(json.dumps(result))


if __name__ == "__main__":
    main()
