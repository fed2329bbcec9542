"""Time of one training step of proqa_amd.trainable_reader.TrainableReader (dev) next to a torch restatement of the
reference's step, at the shape qa/train_dense_qa.sh trains: bert-base, 5 sequences [CLS] q [SEP] p [SEP] of 200-512 tokens,
one question of 12 tokens, P 5000 sampler rows (float32), A 8 answer slots, hidden / attention dropout 0.1, shared norm,
early loss.

    python scripts/dev_reader_step_timing.py [--reps 50] [--trace [--out DIR]]

Default: two contenders take turns in ONE process, a whole step each (forward + backward + optimizer step + zero_grad),
timed with device events (median of --reps after 5 warm-ups of each):
  module  TrainableReader.forward, FusedAdamW.scale_loss(loss).backward(), FusedAdamW.step() (max_grad_norm 2, dynamic scale)
  torch   what a user of the reference has on this GPU: transformers.BertModel (built from a config, no weights read) for
          the reader and the question tower under fp16 autocast, the reference's loss loops (dev_reader_loss_timing's
          restatement: a cross-entropy call per answer position and per gold paragraph, nonzero() three times), GradScaler
          + clip_grad_norm_ + torch.optim.AdamW
The two models have different random weights: the times are comparable, the losses are not.  Prints one JSON line.

--trace: `rocprofv3 --kernel-trace` over a fresh child process that runs the module's step only (a run of its own: no
counters, no other tracing), followed by the embedding backward alone, typed and untyped on the same ids; prints the time
per kernel name and step, and the median of the two embedding kernels.
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
LENS = (512, 377, 512, 200, 448)
QUESTION_PART = 14          # [CLS] + 12 question tokens + [SEP]
P, A = 5000, 8
EMBED_REPS = 20


def make_batch(dev):
    import torch
    g = torch.Generator().manual_seed(13)
    B, S = len(LENS), max(LENS)
    lens = torch.tensor(LENS)
    ar = torch.arange(S)[None]
    mask = ar < lens[:, None]
    ids = torch.randint(1000, 30000, (B, S), generator=g) * mask
    seg = ((ar >= QUESTION_PART) & mask).long()
    pmask = ((ar >= QUESTION_PART) & (ar < lens[:, None] - 1)).long()
    idq = torch.randint(1000, 30000, (1, 12), generator=g).expand(B, 12).contiguous()
    start = torch.full((B, A), -1, dtype=torch.int64)
    end = torch.full((B, A), -1, dtype=torch.int64)
    for b in range(3):                                  # three passages hold the answer, at 1 + b positions
        for a in range(1 + b):
            start[b, a] = 40 + 50 * a + b
            end[b, a] = start[b, a] + 2
    labels = torch.zeros(P, dtype=torch.int64)
    labels[[0, 1, 2, 77, 3100]] = 1
    batch = {"input_ids": ids, "input_mask": mask.long(), "segment_ids": seg, "paragraph_mask": pmask, "input_ids_q": idq,
             "input_mask_q": torch.ones_like(idq), "para_embed": 0.4 * torch.randn(P, 128, generator=g),
             "top5000_labels": labels, "start_positions": start, "end_positions": end, "para_targets": labels[:B].clone()}
    return {k: v.to(dev) for k, v in batch.items()}


class ModuleStep:
    def __init__(self, dev):
        from proqa_amd.optim import FusedAdamW
        from proqa_amd.retriever import BERT_BASE
        from proqa_amd.trainable_reader import TrainableReader
        self.model = TrainableReader(BERT_BASE, device=dev, qa_drop=0.1, hidden_dropout_prob=0.1,
                                     attention_probs_dropout_prob=0.1, dropout_seed=0)
        self.model.freeze_c_encoder()
        self.opt = FusedAdamW([p for p in self.model.parameters() if p.requires_grad], lr=1e-5, max_grad_norm=2.0,
                              loss_scale="dynamic")

    def __call__(self, batch):
        out = self.model(batch)
        self.opt.scale_loss(out["loss"]).backward()
        self.opt.step()
        self.opt.zero_grad()
        return out["loss"].detach()


class TorchStep:
    """The reference's step restated on torch: the baseline, not a product path"""

    def __init__(self, dev):
        import torch
        from transformers import BertConfig, BertModel
        cfg = BertConfig()              # bert-base-uncased's geometry, dropout 0.1
        torch.manual_seed(0)
        self.bert, self.bert_q = BertModel(cfg).to(dev).train(), BertModel(cfg).to(dev).train()
        self.proj_q, self.qa = torch.nn.Linear(768, 128).to(dev), torch.nn.Linear(768, 2).to(dev)
        self.qa_drop = torch.nn.Dropout(0.1)
        self.params = [p for m in (self.bert, self.bert_q, self.proj_q, self.qa) for p in m.parameters()]
        self.opt = torch.optim.AdamW(self.params, lr=1e-5)
        self.scaler = torch.amp.GradScaler("cuda")

    def loss(self, t):
        import torch
        import torch.nn.functional as F
        B, L = t["input_ids"].shape
        hidden = self.bert(t["input_ids"], t["input_mask"], t["segment_ids"])[0]
        logits = self.qa(self.qa_drop(hidden))
        pmask = t["paragraph_mask"].ne(1)
        s, e = (logits[..., k].float().masked_fill(pmask, -1e10).type_as(logits) for k in (0, 1))
        q = self.proj_q(self.bert_q(t["input_ids_q"], t["input_mask_q"])[1])
        rank = q[0].unsqueeze(0).mm(t["para_embed"].type_as(q).t())
        gold = t["top5000_labels"].nonzero()
        per_gold = [F.cross_entropy(rank, g, ignore_index=-1, reduction="none") for g in gold.unbind()]
        early = -torch.log(torch.exp(-torch.cat(per_gold)).sum()) if per_gold else rank.new_zeros(())
        shift = (torch.arange(B, device=s.device) * L).unsqueeze(1)
        sp = (t["start_positions"] + (t["start_positions"] != -1) * shift).view(-1, 1)
        ep = (t["end_positions"] + (t["end_positions"] != -1) * shift).view(-1, 1)
        flat_s, flat_e = s.reshape(1, -1), e.reshape(1, -1)
        ls = [F.cross_entropy(flat_s, p, ignore_index=-1, reduction="none") for p in sp.unbind()]
        le = [F.cross_entropy(flat_e, p, ignore_index=-1, reduction="none") for p in ep.unbind()]
        logp = -(torch.cat(ls) + torch.cat(le)).view(B, A)
        logp = logp.float().masked_fill(logp == 0, float("-inf"))
        marginal = torch.exp(logp).sum(1)
        joint = marginal * F.softmax(rank, -1).view(-1)[:B]
        live = [joint[i] for i in marginal.nonzero()]
        joint_loss = -torch.log(torch.cat(live).sum()) if live else rank.new_zeros(())
        return joint_loss.float() + early.float()

    def __call__(self, batch):
        import torch
        with torch.autocast("cuda", dtype=torch.float16):
            loss = self.loss(batch)
        self.scaler.scale(loss).backward()
        self.scaler.unscale_(self.opt)
        torch.nn.utils.clip_grad_norm_(self.params, 2.0)
        self.scaler.step(self.opt)
        self.scaler.update()
        self.opt.zero_grad(set_to_none=True)
        return loss.detach()


def timed(reps):
    sys.path.insert(0, ROOT)
    import torch
    dev = torch.device("cuda", 0)
    batch = make_batch(dev)
    contenders = {"module": ModuleStep(dev), "torch": TorchStep(dev)}
    times = {k: [] for k in contenders}
    losses = {}
    for i in range(WARMUP + reps):
        for name, step in contenders.items():          # taking turns: both see the same clocks and the same cache history
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            losses[name] = step(batch)
            b.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                times[name].append(a.elapsed_time(b))
    out = {"shape": {"lens": LENS, "question": 12, "P": P, "A": A, "tokens": sum(LENS)}, "reps": reps}
    for name, v in times.items():
        out[name] = {"step_ms_median": statistics.median(v), "step_ms_min": min(v), "last_loss": float(losses[name])}
    out["torch_over_module"] = out["torch"]["step_ms_median"] / out["module"]["step_ms_median"]
    print(json.dumps(out))


def child(reps):
    """under the profiler: the module's steps, then the two embedding backward operators alone on the same ids"""
    sys.path.insert(0, ROOT)
    import torch
    from proqa_amd import trainable as T
    dev = torch.device("cuda", 0)
    batch = make_batch(dev)
    step = ModuleStep(dev)
    for _ in range(WARMUP + reps):
        loss = step(batch)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(5)
    lens = torch.tensor(LENS, dtype=torch.int32)
    cu = torch.zeros(len(LENS) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    half = lambda *shape: (0.02 * torch.randn(*shape, generator=g)).half().to(dev)
    word, pos, types, gamma = half(30522, 768), half(512, 768), half(2, 768), (1.0 + half(768))
    dy = half(sum(LENS), 768)
    for _ in range(EMBED_REPS):
        T.embed_layernorm_typed_backward(dy, batch["input_ids"], batch["segment_ids"], cu.to(dev), word, pos, types, gamma, 1e-12)
        T.embed_layernorm_backward(dy, batch["input_ids"], cu.to(dev), word, pos, types[0].contiguous(), gamma, 1e-12)
    torch.cuda.synchronize()
    print(f"loss={float(loss):.5f}", file=sys.stderr)


def short(name):
    name = name.split("(")[0]
    for tag in ("embed_layernorm_typed_bwd", "attention_dropout_bwd_dq", "attention_dropout_bwd_dkv", "attention_dropout_fwd",
                "bias_residual_layernorm_dropout_bwd", "bias_residual_layernorm_dropout", "dropout_rows",
                "attention_bwd_dq", "attention_bwd_dkv", "attention_fwd", "bias_residual_layernorm_bwd", "bias_residual_layernorm",
                "embed_layernorm_bwd", "embed_layernorm", "column_kernel", "reduce_slabs", "bias_gelu_out", "linear_wgrad",
                "reader_loss_bwd_rows", "reader_loss_bwd_rank", "reader_loss_bwd_sum", "reader_loss_rows", "reader_loss_rank",
                "reader_loss_finish", "reader_loss_pairs", "adamw"):
        if tag in name:
            return tag
    return "gemm (library)" if ("Cijk" in name or "gemm" in name.lower()) else "torch: " + name[-60:]


def trace(reps, out_dir):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if out_dir is None:
        import tempfile
        out_dir = tempfile.mkdtemp(prefix="reader_step_timing_")
    os.makedirs(out_dir, exist_ok=True)
    cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
           "--child", "--reps", str(reps)]
    subprocess.run(cmd, check=True, timeout=900)
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), short(r["Kernel_Name"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    # the stand-alone comparison is the last EMBED_REPS launches of each embedding kernel; the steps end where it begins
    embed = {k: [(t, span) for t, name, span in rows if name == k][-EMBED_REPS:] for k in ("embed_layernorm_typed_bwd", "embed_layernorm_bwd")}
    cutoff = min(v[0][0] for v in embed.values() if v)
    per = {}
    for t, name, span in rows:
        if t < cutoff:
            per[name] = per.get(name, 0) + span
    n = WARMUP + reps
    alone = {k: statistics.median(span for _, span in v) / 1e3 for k, v in embed.items() if v}
    table = {k: v / n / 1e3 for k, v in sorted(per.items(), key=lambda kv: -kv[1])}       # us per step (warm-up included)
    print(json.dumps({"reps": reps, "kernel_us_per_step": dict(list(table.items())[:24]),
                      "kernels_us_per_step_total": sum(table.values()), "embedding_backward_alone_us_median": alone}))


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
