"""What the fused reader objective costs per step next to the reference's way of computing it (dev).

    python scripts/dev_reader_loss_timing.py [--reps 50] [--trace [--out DIR]]

Shape: one question, 5 passages x 512 tokens, hidden 768, P 5000 sampler rows (float32), A 8 answer positions, shared norm,
early loss: the reader step of qa/train_dense_qa.sh.

Default: two contenders take turns in ONE process, forward + backward each, timed with device events around the pair
(median of --reps after 5 warm-ups of each):
  fused   proqa_amd.reader_loss.reader_loss(...)["loss"].backward(): 3 + 4 launches, no host wait
  loops   a torch restatement of how the reference computes the same loss: a half-precision linear, one cross-entropy call
          per answer position and per gold paragraph in Python loops, nonzero() three times (each a host wait), autograd
          backward
Prints one JSON line.  The loops' loss is the reference's (rank scores rounded to fp16, exp in fp32), so the two losses
agree to about 1e-3, which the line reports.

--trace: `rocprofv3 --kernel-trace` over a fresh child process that runs the fused contender only (a run of its own: no
counters, no other tracing); prints the median duration of each of the seven kernels.
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
B, L, H, P, A = 5, 512, 768, 5000, 8
KERNELS = ("reader_loss_rows", "reader_loss_rank", "reader_loss_finish", "reader_loss_pairs", "reader_loss_bwd_rows",
           "reader_loss_bwd_rank", "reader_loss_bwd_sum")


def make_inputs(dev):
    import torch
    g = torch.Generator().manual_seed(512)
    lens = [512, 480, 512, 377, 512]
    offs = [14, 12, 14, 15, 14]
    hidden = torch.randn(B, L, H, generator=g).half()
    start = torch.full((B, A), -1, dtype=torch.int64)
    end = torch.full((B, A), -1, dtype=torch.int64)
    for b in range(3):                                  # three passages hold the answer, at 1 + b positions
        for a in range(1 + b):
            start[b, a] = 40 + 50 * a + b
            end[b, a] = start[b, a] + 2
    labels = torch.zeros(P, dtype=torch.int64)
    labels[[0, 1, 2, 77, 3100]] = 1
    return dict(hidden=hidden.to(dev), lens=lens, offs=offs, qa_w=(0.05 * torch.randn(2, H, generator=g)).to(dev),
                qa_b=torch.zeros(2).to(dev), q=(0.4 * torch.randn(128, generator=g)).half().to(dev),
                para=(0.4 * torch.randn(P, 128, generator=g)).to(dev), labels=labels.to(dev), start=start.to(dev),
                end=end.to(dev))


def fused_step(t):
    import torch
    from proqa_amd.reader_loss import reader_loss
    hidden, w, b, q = (t[k].detach().requires_grad_(True) for k in ("hidden", "qa_w", "qa_b", "q"))
    out = reader_loss(hidden, w, b, q, t["para"], t["labels"], t["start"], t["end"], t["offs_dev"], seq_lens=t["lens_dev"])
    out["loss"].backward()
    return out["loss"].detach()


def loops_step(t):
    """The reference's arithmetic, restated: fp16 linear, masked logits, loops of cross-entropy calls, nonzero()."""
    import torch
    import torch.nn.functional as F
    hidden = t["hidden"].detach().requires_grad_(True)
    w16 = t["qa_w"].half().detach().requires_grad_(True)
    b16 = t["qa_b"].half().detach().requires_grad_(True)
    q = t["q"].detach().requires_grad_(True)
    logits = F.linear(hidden, w16, b16)
    s, e = (logits[..., k].float().masked_fill(~t["pmask"], -1e10).half() for k in (0, 1))
    rank = q.unsqueeze(0).mm(t["para"].half().t())
    gold = t["labels"].nonzero()
    per_gold = [F.cross_entropy(rank, g, ignore_index=-1, reduction="none") for g in gold.unbind()]
    early = -torch.log(torch.exp(-torch.cat(per_gold)).sum()) if per_gold else rank.new_zeros(())
    shift = (torch.arange(B, device=s.device) * L).unsqueeze(1)
    sp = (t["start"] + (t["start"] != -1) * shift).view(-1, 1)
    ep = (t["end"] + (t["end"] != -1) * shift).view(-1, 1)
    flat_s, flat_e = s.reshape(1, -1), e.reshape(1, -1)
    ls = [F.cross_entropy(flat_s, p, ignore_index=-1, reduction="none") for p in sp.unbind()]
    le = [F.cross_entropy(flat_e, p, ignore_index=-1, reduction="none") for p in ep.unbind()]
    logp = -(torch.cat(ls) + torch.cat(le)).view(B, A)
    logp = logp.float().masked_fill(logp == 0, float("-inf"))
    marginal = torch.exp(logp).sum(1)
    joint = marginal * F.softmax(rank, -1).view(-1)[:B]
    live = [joint[i] for i in marginal.nonzero()]
    joint_loss = -torch.log(torch.cat(live).sum()) if live else rank.new_zeros(())
    loss = joint_loss.float() + early.float()
    (loss * 128.0).backward()       # (a loss scale, as amp applies one; 2^16 overflows the fp16 logit gradient here)
    return loss.detach()


def prepare(dev):
    import torch
    t = make_inputs(dev)
    t["lens_dev"] = torch.tensor(t["lens"], dtype=torch.int32, device=dev)
    t["offs_dev"] = torch.tensor(t["offs"], dtype=torch.int32, device=dev)
    pmask = torch.zeros(B, L, dtype=torch.bool)
    for b in range(B):
        pmask[b, t["offs"][b]:t["lens"][b] - 1] = True
    t["pmask"] = pmask.to(dev)
    return t


def timed(reps):
    sys.path.insert(0, ROOT)
    import torch
    dev = torch.device("cuda", 0)
    t = prepare(dev)
    contenders = {"fused": fused_step, "loops": loops_step}
    times = {k: [] for k in contenders}
    losses = {}
    for i in range(WARMUP + reps):
        for name, step in contenders.items():          # taking turns: both see the same clocks and the same cache history
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            losses[name] = step(t)
            b.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                times[name].append(a.elapsed_time(b) * 1e3)
    out = {"shape": {"B": B, "L": L, "H": H, "P": P, "A": A}, "reps": reps}
    for name, v in times.items():
        out[name] = {"us_median": statistics.median(v), "us_min": min(v), "loss": float(losses[name])}
    print(json.dumps(out))


def child(reps):
    sys.path.insert(0, ROOT)
    import torch
    dev = torch.device("cuda", 0)
    t = prepare(dev)
    for _ in range(WARMUP + reps):
        loss = fused_step(t)
    torch.cuda.synchronize()
    print(f"loss={float(loss):.5f}", file=sys.stderr)


def trace(reps, out_dir):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if out_dir is None:
        import tempfile
        out_dir = tempfile.mkdtemp(prefix="reader_loss_timing_")
    os.makedirs(out_dir, exist_ok=True)
    cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
           "--child", "--reps", str(reps)]
    subprocess.run(cmd, check=True, timeout=600)
    spans = {k: [] for k in KERNELS}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for k in KERNELS:
                    if k in r["Kernel_Name"]:           # (no name is a substring of another)
                        spans[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    result = {"reps": reps, "kernels_us_median": {}}
    for k, v in spans.items():
        v.sort()
        if len(v) != WARMUP + reps:
            raise SystemExit(f"expected {WARMUP + reps} launches of {k} in the trace, found {len(v)}")
        result["kernels_us_median"][k] = statistics.median(e - s for s, e in v[WARMUP:]) / 1e3
    result["sum_us"] = sum(result["kernels_us_median"].values())
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None, help="directory of the profiler's output (default: a temporary one)")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    if args.child:
        return child(args.reps)
    if args.trace:
        return trace(args.reps, args.out)
    return timed(args.reps)


if __name__ == "__main__":
    main()
