"""Time of one optimizer step over the parameters of the retriever (dev): proqa_amd.optim.FusedAdamW against the recipe it
replaces and against torch's own fused AdamW.

    python scripts/dev_optimizer_timing.py [--out DIR] [--steps 50] [--skip-trace]

Tensors: the shapes of two bert-base towers and the two projections (proqa_amd.trainable._parameter_shapes: about 219 M
fp32 parameters in about 400 tensors), seeded N(0, 0.02) parameters, seeded gradients N(0, 1e-3) x the loss scale 2^16.
Contenders, all clipping at 2.0 and all with torch.optim.AdamW's update rule:
  fused          FusedAdamW(max_grad_norm=2.0, loss_scale=65536.0, torch_semantics=True).step()
  recipe         GradScaler.unscale_ + clip_grad_norm_ + GradScaler.step(torch.optim.AdamW) + GradScaler.update
  recipe_fused   the same with torch.optim.AdamW(fused=True)
Measurements, each in a fresh child process of this script:
  events   the contenders take turns in one process; every step between device events (the gradients are restored before
           the first event), median of --steps after 5 warm-up rounds; host wall time of the calls next to it;
  trace    `rocprofv3 --kernel-trace` (a run of its own) of ten steps of one contender: kernel time per step; for the
           fused step the three kernels separately, and 32 bytes per parameter (g twice -- the norm and the update --
           p, m, v read once, p, m, v written once; counted from the shapes) over the update + norm kernel time against
           8 TB/s and against proqa_microbench_stream's copy rate on the same box.
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP = 5
TRACE_STEPS = 10
LOSS_SCALE = 65536.0
HBM_SPEC_GBS = 8000.0
CONTENDERS = ("fused", "recipe", "recipe_fused")


def make_tensors(dev, seed):
    import torch
    from proqa_amd.retriever import BERT_BASE, config_from_dict
    from proqa_amd.trainable import _parameter_shapes
    gen = torch.Generator(device=dev).manual_seed(seed)
    shapes = _parameter_shapes(config_from_dict(BERT_BASE))
    return [torch.nn.Parameter(torch.randn(s, generator=gen, device=dev) * 0.02) for s in shapes.values()]


class Contender:
    def __init__(self, name, dev, grads):
        import torch
        self.name, self.grads = name, grads
        self.params = make_tensors(dev, 0)
        for p, g in zip(self.params, grads):
            p.grad = g.clone()
        if name == "fused":
            from proqa_amd.optim import FusedAdamW
            self.opt = FusedAdamW(self.params, lr=1e-5, weight_decay=0.01, max_grad_norm=2.0, loss_scale=LOSS_SCALE,
                                  torch_semantics=True)
        else:
            self.opt = torch.optim.AdamW(self.params, lr=1e-5, weight_decay=0.01, fused=(name == "recipe_fused"))
            self.scaler = torch.amp.GradScaler("cuda", init_scale=LOSS_SCALE, growth_interval=10 ** 9)
            self.scaler.scale(torch.ones((), device=dev))        # creates the scale tensor, as the first scale(loss) does

    def restore_gradients(self):
        import torch
        torch._foreach_copy_([p.grad for p in self.params], self.grads)

    def step(self):
        import torch
        if self.name == "fused":
            self.opt.step()
        else:
            self.scaler.unscale_(self.opt)
            torch.nn.utils.clip_grad_norm_(self.params, 2.0)
            self.scaler.step(self.opt)
            self.scaler.update()


def child(mode, names, steps):
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
        out, v = {}, ctypes.c_double()
        for key, kind in (("hbm_copy_GBs", 0), ("hbm_read_GBs", 1)):
            _lib.check(lib.proqa_microbench_stream(buf.data_ptr(), nbytes, kind, 5, _lib.current_stream_ptr(), ctypes.byref(v)))
            out[key] = v.value
        print("RESULT " + json.dumps(out))
        return
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(p.shape, generator=gen, device=dev) * (1e-3 * LOSS_SCALE) for p in make_tensors(dev, 0)]
    contenders = [Contender(n, dev, grads) for n in names]
    n_params = sum(g.numel() for g in grads)
    result = {"parameters": n_params, "tensors": len(grads), "bytes_per_step": 32 * n_params}
    if mode == "trace":
        for c in contenders:          # (no gradient restore: nothing but the step's own kernels in the trace)
            for _ in range(TRACE_STEPS):
                c.step()
        torch.cuda.synchronize()
        print("RESULT " + json.dumps(result))
        return
    device_ms = {c.name: [] for c in contenders}
    host_ms = {c.name: [] for c in contenders}
    for _ in range(WARMUP + steps):
        for c in contenders:
            c.restore_gradients()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            c.step()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            device_ms[c.name].append(e0.elapsed_time(e1))
            host_ms[c.name].append((t1 - t0) * 1e3)
    for c in contenders:
        d, h = device_ms[c.name][WARMUP:], host_ms[c.name][WARMUP:]
        result[c.name] = {"step_ms_median": statistics.median(d), "step_ms_min": min(d), "step_ms_max": max(d),
                          "host_call_ms_median": statistics.median(h), "steps": len(d)}
    fused = next((c for c in contenders if c.name == "fused"), None)
    if fused is not None:
        result["fused"]["last_grad_norm"] = float(fused.opt.last_grad_norm)
        result["fused"]["state"] = fused.opt.state_dict()["fused"]
    print("RESULT " + json.dumps(result))


def run_child(mode, names, steps, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", mode, "--contenders", ",".join(names),
                          "--steps", str(steps)]
    try:
        out = subprocess.run(cmd, check=True, timeout=900, capture_output=True, text=True).stdout
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
    ap.add_argument("--contenders", default=",".join(CONTENDERS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--skip-trace", action="store_true")
    args = ap.parse_args()
    names = args.contenders.split(",")
    if args.child:
        return child(args.child, names, args.steps)
    if args.steps < 50:
        print("note: fewer than 50 timed steps", file=sys.stderr)
    result = {"events": run_child("events", names, args.steps), "stream": run_child("stream", names, args.steps)}
    if not args.skip_trace:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if args.out is None:
            import tempfile
            args.out = tempfile.mkdtemp(prefix="optimizer_timing_")
        nbytes = result["events"]["bytes_per_step"]
        trace = {}
        for name in names:              # one traced run per contender, so that its kernels are the whole trace
            d = os.path.join(args.out, name)
            os.makedirs(d, exist_ok=True)
            run_child("trace", [name], args.steps, prefix=[prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
            per = read_trace(d)
            if name == "fused":
                ours = {}
                for tag in ("adamw_grad_sumsq", "adamw_finalize", "adamw_update"):
                    times = [t for k, v in per.items() if tag in k for t in v]
                    ours[tag + "_us_median"] = statistics.median(times) / 1e3 if times else None
                    ours[tag + "_launches"] = len(times)
                stream_us = (ours["adamw_grad_sumsq_us_median"] or 0.0) + (ours["adamw_update_us_median"] or 0.0)
                ours["kernel_us_per_step"] = stream_us + (ours["adamw_finalize_us_median"] or 0.0)
                if stream_us:
                    gbs = nbytes / (stream_us * 1e-6) / 1e9
                    ours["GBs_over_the_two_streaming_kernels"] = gbs
                    ours["fraction_of_8TBs"] = gbs / HBM_SPEC_GBS
                    ours["fraction_of_measured_copy_rate"] = gbs / result["stream"]["hbm_copy_GBs"]
                trace[name] = ours
            else:
                # the first steps create the optimizer state: per-step figures from all launches are slightly high
                total = sum(sum(v) for v in per.values())
                trace[name] = {"kernel_us_per_step": total / TRACE_STEPS / 1e3,
                               "launches_per_step": sum(len(v) for v in per.values()) / TRACE_STEPS}
        result["trace"] = trace
    print(json.dumps(result))


if __name__ == "__main__":
    main()
