"""Time of one forward + backward step of proqa_amd.trainable.TrainableRetriever (dev), bert-base on seeded synthetic
batches at the reference's --train_batch_size 640 (retrieval/train_retriever_single.sh) and at 64.

    python scripts/dev_train_step_timing.py [--out DIR] [--batches 640,64] [--steps 5] [--skip-trace] [--dropout P]
                                            [--deterministic] [--half-weights [--accumulate N]]
                                            [--micro-batches-per-pass 1,4,8 [--accumulate N]]

Three measurements, each in a fresh child process of this script:
  events   forward + backward + zero_grad per step between CUDA events, median of --steps after 2 warm-up steps;
  torch    the same step by torch autograd over an fp16 restatement of the tower on the same GPU (padded layout,
           torch.softmax attention): what a user had before this module;
  trace    `rocprofv3 --kernel-trace` (a run of its own: no counters, no other tracing) over the module's steps: time per
           kernel name and step, and the attention backward's fraction of the fp16 dense peak from the flops its shapes
           imply (five products of 2 L^2 64 per (sequence, head); the kernels execute nine).
--dropout P (what BERT's dropout costs): the module is built with both rates P; in `events` and `trace` a step with
dropout and a step without (the rates set to 0: the dropout-free kernels) take turns in one process, each --steps times
after the warm-up.  `events` adds step_ms_median_dropout and dropout_step_ratio; `trace` adds dropout_kernel_ratios: the
time of each dropout kernel over its dropout-free counterpart (the three attention kernels and the LayerNorm pair).
--deterministic (what the fixed-order word-embedding gradient costs in a step): in `events` a step of the default module
and a step with deterministic=True take turns in one process; adds step_ms_median_deterministic and
deterministic_step_ratio.  Not combined with --dropout; the trace is of the default module.
--half-weights (what the fp16 working copies are worth): the step becomes --accumulate N micro-batches of forward +
backward, one FusedAdamW step (clip 2.0, dynamic scale) and zero_grad.  Two modules of the same weights take turns in one
process, one casting its masters in every forward, the other with half_weights() and FusedAdamW(half_copies=...): `events`
gives step_ms_median_casts / _copies and their ratio; `trace` runs each variant in a traced process of its own and gives
launches per micro-batch, the adamw_update time and the time of the cast kernels.  The torch baseline is skipped.
--micro-batches-per-pass 1,4,8 (what pretrain_retriever.py's flag of that name is worth): the step is one accumulation
window of --accumulate N micro-batches of (first of --batches) / N pairs each, every micro-batch with seeded lengths of its
own, one FusedAdamW step with the fp16 working copies and zero_grad.  At setting M the window's micro-batches go through
the towers M at a time: one forward on the list, inbatch_loss_blocks, one backward; M = 1 is the command's route without
the flag (inbatch_loss per micro-batch), the yardstick.  `events`: the settings take turns step by step in one process,
device events, medians, peak allocated memory per setting; `trace`: one traced process per setting gives launches and
kernel time per step.  The torch baseline is skipped.
Questions have 5-30 tokens (--max_query_length 30), paragraphs 60-220.  Prints one JSON line.
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
WARMUP = 2
PEAK_TFLOPS = 2500.0      # fp16 dense, MI355X


def make_batch(pairs, seed, dev):
    import torch
    g = torch.Generator().manual_seed(seed)
    lq = torch.randint(5, 31, (pairs,), generator=g)
    lc = torch.randint(60, 221, (pairs,), generator=g)
    out = {}
    for side, lens in (("q", lq), ("c", lc)):
        S = int(lens.max())
        ids = torch.randint(1000, 30000, (pairs, S), generator=g)
        mask = torch.arange(S)[None] < lens[:, None]
        out[f"input_ids_{side}"] = (ids * mask).to(dev)
        out[f"input_mask_{side}"] = mask.to(dev)
    return out, lq.tolist(), lc.tolist()


def attention_flops(lens, n_heads, n_layers):
    return sum(5 * 2.0 * n * n * 64 for n in lens) * n_heads * n_layers


class TorchTower:
    """fp16 restatement on torch (padded layout): the baseline, not a product path"""

    def __init__(self, model):
        self.model = model

    def tower(self, tower, proj, ids, mask):
        import torch
        import torch.nn.functional as F
        P, cfg = self.model._flat, self.model.config
        h16 = lambda k: P[k].half()
        B, S = ids.shape
        e = f"{tower}.embeddings"
        x = h16(f"{e}.word_embeddings.weight")[ids] + h16(f"{e}.position_embeddings.weight")[:S][None] \
            + h16(f"{e}.token_type_embeddings.weight")[0]
        H = x.shape[-1]
        h = F.layer_norm(x, (H,), h16(f"{e}.LayerNorm.weight"), h16(f"{e}.LayerNorm.bias"), cfg.layer_norm_eps)
        add = torch.where(mask, 0.0, -65504.0).half()[:, None, None, :]
        nh = cfg.num_attention_heads
        for i in range(cfg.num_hidden_layers):
            p = f"{tower}.encoder.layer.{i}"
            lin = lambda name, t: F.linear(t, h16(f"{p}.{name}.weight"), h16(f"{p}.{name}.bias"))
            q, k, v = (lin(f"attention.self.{n}", h).view(B, S, nh, 64).transpose(1, 2) for n in ("query", "key", "value"))
            probs = torch.softmax(q @ k.transpose(-1, -2) * 0.125 + add, -1)
            ctx = (probs @ v).transpose(1, 2).reshape(B, S, H)
            h1 = F.layer_norm(lin("attention.output.dense", ctx) + h, (H,), h16(f"{p}.attention.output.LayerNorm.weight"),
                              h16(f"{p}.attention.output.LayerNorm.bias"), cfg.layer_norm_eps)
            f = F.gelu(lin("intermediate.dense", h1))
            h = F.layer_norm(lin("output.dense", f) + h1, (H,), h16(f"{p}.output.LayerNorm.weight"),
                             h16(f"{p}.output.LayerNorm.bias"), cfg.layer_norm_eps)
        pooled = torch.tanh(F.linear(h[:, 0], h16(f"{tower}.pooler.dense.weight"), h16(f"{tower}.pooler.dense.bias")))
        return F.linear(pooled, h16(f"{proj}.weight"), h16(f"{proj}.bias"))

    def __call__(self, batch):
        return {"q": self.tower("bert_q", "proj_q", batch["input_ids_q"], batch["input_mask_q"]),
                "c": self.tower("bert_c", "proj_c", batch["input_ids_c"], batch["input_mask_c"])}


def child(mode, batches, steps, dropout=0.0, deterministic=False):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from proqa_amd.retriever import BERT_BASE
    from proqa_amd.trainable import TrainableRetriever, inbatch_loss
    dev = torch.device("cuda", 0)
    model = TrainableRetriever(BERT_BASE, device=dev, dropout_seed=0)
    turns = [0.0, dropout] if dropout > 0 and mode != "torch" else [0.0]
    fixed_order = [False, True] if deterministic and mode == "events" and len(turns) == 1 else [False]
    turns = turns * len(fixed_order)
    result = {}
    for pairs in batches:
        batch, lq, lc = make_batch(pairs, pairs, dev)
        forward = TorchTower(model) if mode == "torch" else model
        times = []
        for step in range((WARMUP + steps) * len(turns)):
            model.hidden_dropout_prob = model.attention_probs_dropout_prob = turns[step % len(turns)]
            model.deterministic = fixed_order[step % len(fixed_order)]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = forward(batch)
            if mode == "torch":
                loss = F.cross_entropy((out["q"] @ out["c"].t()).float(), torch.arange(pairs, device=dev))
            else:
                loss = inbatch_loss(out["q"], out["c"])
            (loss * 1024.0).backward()
            model.zero_grad(set_to_none=True)
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1))
        plain = times[0::len(turns)][WARMUP:]
        result[str(pairs)] = {"step_ms_median": statistics.median(plain), "step_ms_min": min(plain),
                              "loss": float(loss), "tokens": sum(lq) + sum(lc),
                              "attention_backward_flops": attention_flops(lq, 12, 12) + attention_flops(lc, 12, 12)}
        if len(fixed_order) > 1:
            fixed = times[1::2][WARMUP:]
            result[str(pairs)].update(step_ms_median_deterministic=statistics.median(fixed),
                                      deterministic_step_ratio=statistics.median(fixed) / statistics.median(plain))
        elif len(turns) > 1:
            dropped = times[1::2][WARMUP:]
            result[str(pairs)].update(dropout=dropout, step_ms_median_dropout=statistics.median(dropped),
                                      dropout_step_ratio=statistics.median(dropped) / statistics.median(plain))
    print("RESULT " + json.dumps(result))


def child_half(mode, batches, steps, accumulate, variant):
    """--half-weights: optimizer steps of `accumulate` micro-batches, per-forward casts and working copies taking turns
    (variant None) or one of them alone (a traced run)"""
    sys.path.insert(0, ROOT)
    import torch
    from proqa_amd.optim import FusedAdamW
    from proqa_amd.retriever import BERT_BASE
    from proqa_amd.trainable import TrainableRetriever, inbatch_loss
    dev = torch.device("cuda", 0)
    names = ["casts", "copies"] if variant is None else [variant]
    models, opts = {}, {}
    for name in names:
        model = TrainableRetriever(BERT_BASE, device=dev, dropout_seed=0)
        kw = dict(half_copies=model.half_weights()) if name == "copies" else {}
        models[name] = model
        opts[name] = FusedAdamW(model.parameters(), lr=1e-5, max_grad_norm=2.0, loss_scale="dynamic", **kw)
    result = {}
    for pairs in batches:
        batch, lq, lc = make_batch(pairs, pairs, dev)
        times = {name: [] for name in names}
        for step in range((WARMUP + steps) * len(names)):
            name = names[step % len(names)]
            model, opt = models[name], opts[name]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(accumulate):
                out = model(batch)
                loss = inbatch_loss(out["q"], out["c"]) / accumulate
                opt.scale_loss(loss).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1))
        med = {name: statistics.median(t[WARMUP:]) for name, t in times.items()}
        result[str(pairs)] = {"accumulate": accumulate, "loss": float(loss), "tokens": sum(lq) + sum(lc),
                              **{f"step_ms_median_{name}": v for name, v in med.items()},
                              **{f"step_ms_min_{name}": min(t[WARMUP:]) for name, t in times.items()}}
        if len(names) == 2:
            result[str(pairs)]["copies_over_casts"] = med["copies"] / med["casts"]
    print("RESULT " + json.dumps(result))


def child_passes(mode, pairs, steps, accumulate, settings):
    """--micro-batches-per-pass: optimizer steps over one window of `accumulate` micro-batches, the settings taking turns"""
    sys.path.insert(0, ROOT)
    import torch
    from proqa_amd.optim import FusedAdamW
    from proqa_amd.retriever import BERT_BASE
    from proqa_amd.trainable import TrainableRetriever, inbatch_loss, inbatch_loss_blocks
    dev = torch.device("cuda", 0)
    model = TrainableRetriever(BERT_BASE, device=dev, dropout_seed=0)
    opt = FusedAdamW(model.parameters(), lr=1e-5, max_grad_norm=2.0, loss_scale="dynamic", half_copies=model.half_weights())
    micro = pairs // accumulate
    made = [make_batch(micro, 1000 + m, dev) for m in range(accumulate)]
    window = [b for b, _, _ in made]
    tokens = sum(sum(lq) + sum(lc) for _, lq, lc in made)
    times, peak, losses = {M: [] for M in settings}, {M: 0 for M in settings}, {}
    for step in range((WARMUP + steps) * len(settings)):
        M = settings[step % len(settings)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        seen = []
        for at in range(0, accumulate, M):
            group = window[at:at + M]
            if len(group) == 1:
                out = model(group[0])
                loss = inbatch_loss(out["q"], out["c"]) / accumulate
                opt.scale_loss(loss).backward()
                seen.append(loss.detach().reshape(1))
            else:
                out = model(group)
                per = inbatch_loss_blocks(out["q"], out["c"], out["block_sizes"]) / accumulate
                opt.scale_loss(per.sum()).backward()
                seen.append(per.detach())
        opt.step()
        opt.zero_grad(set_to_none=True)
        t1.record()
        torch.cuda.synchronize()
        times[M].append(t0.elapsed_time(t1))
        peak[M] = max(peak[M], torch.cuda.max_memory_allocated(dev))
        losses[M] = float(torch.cat(seen).sum())
    result = {"pairs": pairs, "accumulate": accumulate, "micro_batch_pairs": micro, "tokens_per_step": tokens, "settings": {}}
    for M in settings:
        t = times[M][WARMUP:]
        result["settings"][str(M)] = {"step_ms_median": statistics.median(t), "step_ms_min": min(t), "step_ms_all": t,
                                      "passes_per_step": -(-accumulate // M), "peak_allocated_bytes": peak[M],
                                      "window_loss": losses[M]}
    print("RESULT " + json.dumps(result))


def main_passes(args, batches):
    settings = [int(m) for m in args.micro_batches_per_pass.split(",")]
    base = [sys.executable, os.path.abspath(__file__), "--batches", str(batches[0]), "--steps", str(args.steps), "--accumulate",
            str(args.accumulate)]

    def run(mode, which, prefix=()):
        cmd = list(prefix) + base + ["--child", mode, "--micro-batches-per-pass", ",".join(str(m) for m in which)]
        out = subprocess.run(cmd, check=True, timeout=900, capture_output=True, text=True).stdout
        return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])

    result = {"rocm": open("/opt/rocm/.info/version").read().strip() if os.path.exists("/opt/rocm/.info/version") else "",
              "events": run("events", settings)}
    ref = result["events"]["settings"][str(settings[0])]["step_ms_median"]
    for M in settings:
        result["events"]["settings"][str(M)]["over_first_setting"] = result["events"]["settings"][str(M)]["step_ms_median"] / ref
    if not args.skip_trace:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if args.out is None:
            import tempfile
            args.out = tempfile.mkdtemp(prefix="train_step_timing_")
        trace = {}
        for M in settings:                      # one traced run per setting: its kernels are the whole trace
            d = os.path.join(args.out, f"passes_{M}")
            os.makedirs(d, exist_ok=True)
            run("trace", [M], prefix=[prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
            rows = read_trace(d)
            n = WARMUP + args.steps
            per = {}
            for name, s, e in rows:
                per[short(name)] = per.get(short(name), 0) + (e - s)
            table = {k: v / n / 1e3 for k, v in sorted(per.items(), key=lambda kv: -kv[1])}
            trace[str(M)] = {"launches_per_step": len(rows) / n, "kernels_us_per_step_total": sum(table.values()),
                             "kernel_us_per_step": dict(list(table.items())[:12])}
        result["trace"] = trace
    print(json.dumps(result))


def run_child(mode, args, prefix=(), variant=None):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", mode, "--batches", args.batches, "--steps", str(args.steps),
                          "--dropout", str(args.dropout)]
    if getattr(args, "deterministic", False):
        cmd += ["--deterministic"]
    if getattr(args, "half_weights", False):
        cmd += ["--half-weights", "--accumulate", str(args.accumulate)] + (["--variant", variant] if variant else [])
    out = subprocess.run(cmd, check=True, timeout=900, capture_output=True, text=True).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def read_trace(out_dir):
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort(key=lambda r: r[1])
    return rows


def short(name):
    name = name.split("(")[0]
    for tag in ("attention_dropout_bwd_dq", "attention_dropout_bwd_dkv", "attention_dropout_fwd", "bias_residual_layernorm_dropout_bwd",
                "bias_residual_layernorm_dropout", "dropout_rows",
                "attention_bwd_dq", "attention_bwd_dkv", "attention_fwd", "bias_residual_layernorm_bwd", "bias_residual_layernorm",
                "embed_layernorm_bwd", "embed_layernorm", "column_kernel", "reduce_slabs", "bias_gelu_out",
                "inbatch_loss_blocks_grad", "inbatch_loss_grad", "inbatch_eval_blocks", "inbatch_block_loss", "inbatch_eval"):
        if tag in name:
            return tag
    return "gemm (library)" if ("Cijk" in name or "gemm" in name.lower()) else "torch: " + name[-60:]


def main_half(args, batches):
    result = {"rocm": open("/opt/rocm/.info/version").read().strip() if os.path.exists("/opt/rocm/.info/version") else "",
              "accumulate": args.accumulate, "module": run_child("events", args)}
    if not args.skip_trace:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if args.out is None:
            import tempfile
            args.out = tempfile.mkdtemp(prefix="train_step_timing_")
        trace = {}
        for b in batches:
            for variant in ("casts", "copies"):      # one traced run per size and variant: its kernels are the whole trace
                d = os.path.join(args.out, f"{b}_{variant}")
                os.makedirs(d, exist_ok=True)
                one = argparse.Namespace(batches=str(b), steps=args.steps, dropout=0.0, half_weights=True, accumulate=args.accumulate)
                run_child("trace", one, prefix=[prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--"], variant=variant)
                rows = read_trace(d)
                n = WARMUP + args.steps
                us = lambda pred: sum(e - s for name, s, e in rows if pred(name)) / n / 1e3
                trace.setdefault(str(b), {})[variant] = {
                    "launches_per_micro_batch": len(rows) / n / args.accumulate,      # (the optimizer's few launches included)
                    "adamw_update_us_per_step": us(lambda k: "adamw_update" in k),
                    "adamw_us_per_step": us(lambda k: "adamw_" in k),
                    "kernels_us_per_step_total": us(lambda k: True)}
        result["trace"] = trace
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, choices=["events", "torch", "trace"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="640,64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--dropout", type=float, default=0.0, help="also time steps with both dropout rates at this value")
    ap.add_argument("--deterministic", action="store_true", help="also time steps with the word-embedding gradient in a fixed order")
    ap.add_argument("--half-weights", action="store_true", help="optimizer steps with and without the fp16 working copies")
    ap.add_argument("--accumulate", type=int, default=1, help="micro-batches per optimizer step (with --half-weights)")
    ap.add_argument("--micro-batches-per-pass", default=None,
                    help="e.g. 1,4,8: optimizer steps over one window of --accumulate micro-batches, M per tower pass")
    ap.add_argument("--variant", default=None, choices=["casts", "copies"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    if args.micro_batches_per_pass:
        settings = [int(m) for m in args.micro_batches_per_pass.split(",")]
        if args.child:
            return child_passes(args.child, batches[0], args.steps, args.accumulate, settings)
        return main_passes(args, batches)
    if args.child and args.half_weights:
        return child_half(args.child, batches, args.steps, args.accumulate, args.variant)
    if args.child:
        return child(args.child, batches, args.steps, args.dropout, args.deterministic)
    if args.half_weights:
        return main_half(args, batches)
    result = {"rocm": open("/opt/rocm/.info/version").read().strip() if os.path.exists("/opt/rocm/.info/version") else "",
              "module": run_child("events", args), "torch_autograd_fp16": run_child("torch", args)}
    if not args.skip_trace:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if args.out is None:
            import tempfile
            args.out = tempfile.mkdtemp(prefix="train_step_timing_")
        per_batch = {}
        for b in batches:      # one traced run per batch size, so that the kernels of a size are the whole trace
            d = os.path.join(args.out, str(b))
            os.makedirs(d, exist_ok=True)
            one = argparse.Namespace(batches=str(b), steps=args.steps, dropout=args.dropout)
            info = run_child("trace", one, prefix=[prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--"])[str(b)]
            per = {}
            for name, s, e in read_trace(d):
                per[short(name)] = per.get(short(name), 0) + (e - s)
            n = WARMUP + args.steps
            table = {k: v / n / 1e3 for k, v in sorted(per.items(), key=lambda kv: -kv[1])}      # us per step (warm-up included)
            att_us = table.get("attention_bwd_dq", 0.0) + table.get("attention_bwd_dkv", 0.0)
            per_batch[str(b)] = {"kernel_us_per_step": dict(list(table.items())[:16]), "kernels_us_per_step_total": sum(table.values()),
                                 "attention_backward_us_per_step": att_us,
                                 "attention_backward_fraction_of_fp16_peak": info["attention_backward_flops"] / (att_us * 1e-6) / 1e12 / PEAK_TFLOPS if att_us else None}
            if args.dropout > 0:       # (both kinds of step ran n times each in the traced process)
                pairs = {"attention_fwd": "attention_dropout_fwd", "attention_bwd_dq": "attention_dropout_bwd_dq",
                         "attention_bwd_dkv": "attention_dropout_bwd_dkv", "bias_residual_layernorm": "bias_residual_layernorm_dropout",
                         "bias_residual_layernorm_bwd": "bias_residual_layernorm_dropout_bwd"}
                per_batch[str(b)]["dropout_kernel_ratios"] = {k: table[v] / table[k] for k, v in pairs.items() if k in table and v in table}
                per_batch[str(b)]["dropout_kernel_us_per_step"] = {v: table.get(v) for v in list(pairs.values()) + ["dropout_rows"]}
        result["trace"] = per_batch
    print(json.dumps(result))


if __name__ == "__main__":
    main()
