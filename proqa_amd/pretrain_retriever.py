"""`python pretrain_retriever.py --train_file train.txt --predict_file dev.txt --bert_model_name DIR ...`: retriever
pre-training, the loop of retrieval/train_retriever.py:32-285 on one MI355X.

Same flags (proqa_amd.config), same output directory and model_name, same accumulation rule, evaluation, checkpoints
(checkpoint_{step}.pt, checkpoint_last.pt, checkpoint_best.pt: model.state_dict(), fp32, the reference's keys) and
early-stopping counter.  The model is TrainableRetriever with the config's two dropout rates, the optimizer FusedAdamW
with the reference's two parameter groups, a dynamic loss scale, the clip of --max_grad_norm inside the fused step, and
the fp16 working copies of the weight matrices written by that step (TrainableRetriever.half_weights()).

Intended differences: activations are fp16 with or without --fp16 and --fp16_opt_level is ignored;
batches are tokenised in this process (ReTextView + ReTokenizeCollate), no worker is forked once the GPU is initialised;
the host never reads a loss inside the loop: the per-micro-batch losses stay on the device and are read at evaluation
and checkpoint time and at the end; the initial BERT weights come from the local --bert_model_name directory only (nothing
is fetched); --local_rank, --no_cuda and a ';' list in --init_checkpoint are refused.  `train_retriever.py --do_train` keeps
its refusal; `--do_predict` alone belongs to that command.

Beyond the reference (proqa_amd/checkpoint.py): --save-state writes trainer_state_last.pt (masters,
AdamW moments, counters, sampler position, RNG and dropout state) behind the training stream, --stop-after-updates K stops
after the K-th update with the state written, --resume PATH continues from it (with --deterministic to the bits of the
uninterrupted run), --digest-every N records 64-bit digests of the masters and both moments.  Without these flags the
command writes the files, log lines and stats keys it always wrote.
"""
import json
import logging
import os
import time

from .trainer import TrainerRun, check_train_args, seed_everything, tensorboard

LAST_RUN_STATS = {}

# test hook: parameters whose name contains one of these substrings are frozen (without --deterministic the word-embedding
# gradient is summed with atomics, the module's one run-to-run difference; frozen, or with --deterministic, two runs of one
# seed log identical losses)
FROZEN_PARAMETERS = ()

logger = logging.getLogger(__name__)


# ---- pure pieces (no GPU) ------------------------------------------------------------------------------------------------

def model_name(args):
    """the reference's run name (train_retriever.py:44-45), from the flags BEFORE train_batch_size is divided"""
    data_name = args.train_file.split("/")[-1].split("-")[0]
    return (f"{data_name}-seed{args.seed}-bsz{args.train_batch_size}-fp16{args.fp16}-{args.prefix}-lr{args.learning_rate}-"
            f"{args.bert_model_name}-filter{args.filter}")


def check_args(args):
    """The refusals, and --do_train implied.  Raises what the reference raises where it raises."""
    check_train_args(args, "pretrain_retriever.py", "the dev evaluation of a checkpoint: run train_retriever.py")
    if ";" in args.init_checkpoint:
        raise SystemExit("pretrain_retriever.py: a ';' list in --init_checkpoint (the reference's ensemble path) is not "
                         "supported; training starts from one checkpoint")
    if int(args.train_batch_size / args.accumulate_gradients) < 1:
        raise ValueError(f"--train_batch_size {args.train_batch_size} / --accumulate_gradients {args.accumulate_gradients} "
                         "leaves no example per batch")
    if args.micro_batches_per_pass < 1:
        raise SystemExit(f"pretrain_retriever.py: --micro-batches-per-pass {args.micro_batches_per_pass}: must be at least 1")
    from .config import check_state_flags
    return check_state_flags(args, "pretrain_retriever.py")


def batch_slices(order, batch_size):
    """What DataLoader(batch_size=..., sampler=...) yields: consecutive slices of the sampler's order, the short last one
    kept."""
    order = list(order)
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


def is_update_step(batch_step, gradient_accumulation_steps):
    """The reference's rule (train_retriever.py:222), batch_step counted from 1 (it is incremented before the forward):
    with G = 2 the first update follows ONE micro-batch (batch_step 1), every later one two."""
    return (batch_step + 1) % gradient_accumulation_steps == 0


def update_schedule(n_batches, gradient_accumulation_steps):
    """[batch_step of every optimizer step] over n_batches micro-batches"""
    return [b for b in range(1, n_batches + 1) if is_update_step(b, gradient_accumulation_steps)]


def pass_schedule(n_batches, gradient_accumulation_steps, micro_batches_per_pass, first=1):
    """[[batch_step of every micro-batch of the pass]] over ONE epoch of n_batches micro-batches whose batch steps are
    first .. first + n_batches - 1 (--micro-batches-per-pass): a pass holds consecutive micro-batches and closes when it
    holds micro_batches_per_pass of them, at an update step (the optimizer step needs every gradient of its window and the
    next micro-batch reads the new weights) or with the epoch.  The accumulation rule is the reference's: with G = 8 the
    first update follows seven micro-batches, so the first window's passes hold seven between them."""
    passes, open_pass = [], []
    for b in range(first, first + n_batches):
        open_pass.append(b)
        if len(open_pass) >= micro_batches_per_pass or is_update_step(b, gradient_accumulation_steps):
            passes.append(open_pass)
            open_pass = []
    if open_pass:
        passes.append(open_pass)
    return passes


def fingerprint_extra(args):
    """The command's own field of the resume fingerprint: micro_batches_per_pass, only when it is not 1, so that the state
    files of one-micro-batch passes keep their fingerprint (the rule of train_reader.py's questions_per_pass)."""
    M = int(getattr(args, "micro_batches_per_pass", 1))
    return {"micro_batches_per_pass": M} if M != 1 else {}


def check_micro_batches_per_pass(saved_fingerprint, value):
    """SystemExit when the state file was written at another --micro-batches-per-pass (a state file without the field was
    written at 1, where check_fingerprint would pass over the field)."""
    was = int(saved_fingerprint.get("micro_batches_per_pass", 1))
    if was != int(value):
        raise SystemExit(f"--resume: the state file was written by a different run: field 'micro_batches_per_pass' is "
                         f"{int(value)!r} now, was {was!r} when the state was saved")


def load_bert_weights(model_dir):
    """{bare BertModel key: tensor} from pytorch_model.bin (or model.safetensors if that package imports) of a LOCAL model
    directory; a 'bert.' prefix (BertForPreTraining checkpoints) is stripped, heads that are not BertModel's are dropped.
    SystemExit when the directory holds no weights: nothing is ever fetched."""
    import torch
    path_bin = os.path.join(model_dir, "pytorch_model.bin")
    path_st = os.path.join(model_dir, "model.safetensors")
    sd = None
    if os.path.isfile(path_bin):
        sd = torch.load(path_bin, map_location="cpu")
    elif os.path.isfile(path_st):
        try:
            from safetensors.torch import load_file
        except ImportError:
            load_file = None
        if load_file is not None:
            sd = load_file(path_st)
    if sd is None:
        raise SystemExit(f"pretrain_retriever.py: no BERT weights in {model_dir!r} (pytorch_model.bin, or model.safetensors "
                         "with the safetensors package) and no --init_checkpoint: nothing to start from; weights are "
                         "never downloaded")
    out = {}
    for k, v in sd.items():
        if k.startswith("bert."):
            k = k[len("bert."):]
        if k.startswith(("embeddings.", "encoder.", "pooler.")) and not k.endswith("position_ids"):
            out[k] = v
    return out


def initial_state_dict(cfg, bert_weights, seed):
    """The reference's untrained retriever: both towers are the pre-trained BertModel, the projections nn.Linear's
    initialisation (under `seed`)."""
    import torch
    from ._lib import EMBED_DIM
    from .retriever import tower_keys
    sd = {}
    for tower in ("bert_q", "bert_c"):
        for key in tower_keys(tower, cfg.num_hidden_layers):
            bare = key[len(tower) + 1:]
            if bare not in bert_weights:
                raise SystemExit(f"pretrain_retriever.py: the BERT weights lack {bare!r}")
            sd[key] = bert_weights[bare].detach().to(torch.float32).clone()
    torch.manual_seed(seed)
    for proj in ("proj_q", "proj_c"):
        lin = torch.nn.Linear(cfg.hidden_size, EMBED_DIM)
        sd[f"{proj}.weight"], sd[f"{proj}.bias"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    return sd


def load_model_config(name_or_dir):
    """(config namespace, hidden_dropout_prob, attention_probs_dropout_prob) of a model directory's config.json (else of
    transformers' local files); the two rates default to BertConfig's 0.1"""
    from .retriever import config_from_dict
    cfg_path = os.path.join(name_or_dir, "config.json")
    if os.path.isfile(cfg_path):
        with open(cfg_path) as f:
            d = json.load(f)
    else:
        from transformers import BertConfig
        d = BertConfig.from_pretrained(name_or_dir, local_files_only=True).to_dict()
    return config_from_dict(d), float(d.get("hidden_dropout_prob", 0.1)), float(d.get("attention_probs_dropout_prob", 0.1))


def parameter_groups(model, weight_decay):
    """The reference's two groups (train_retriever.py:140-146), without the parameters that do not train"""
    no_decay = ["bias", "LayerNorm.weight"]
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    return [{"params": [p for n, p in named if not any(nd in n for nd in no_decay)], "weight_decay": weight_decay},
            {"params": [p for n, p in named if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]


# ---- the command -------------------------------------------------------------------------------------------------------------

def main(argv=None):
    from .config import get_args
    args = check_args(get_args(argv))
    import torch
    from transformers import BertTokenizer
    from .datasets import ClusterDataset, ClusterSampler, ReDataset, ReSampler, ReTextView, ReTokenizeCollate
    from .get_embed import usable_cpus
    from .optim import FusedAdamW
    from .train_retriever import predict
    from .trainable import TrainableRetriever, inbatch_loss, inbatch_loss_blocks
    from .utils import move_to_cuda

    name = model_name(args)
    tb_dir = os.path.join(args.output_dir, "tflogs", name)
    args.output_dir = os.path.join(args.output_dir, name)
    with TrainerRun("pretrain_retriever.py", args, logger) as run:
        logger.info(args)
        if not torch.cuda.is_available():
            raise RuntimeError("no MI355X visible: retriever training has no CPU fallback")
        flag_batch_size = args.train_batch_size
        args.train_batch_size = int(args.train_batch_size / args.accumulate_gradients)
        seed_everything(args.seed)

        cfg, p_hidden, p_attention = load_model_config(args.bert_model_name)
        if args.max_seq_length > cfg.max_position_embeddings:
            raise ValueError("Cannot use sequence length %d because the BERT model was only trained up to sequence length %d"
                             % (args.max_seq_length, cfg.max_position_embeddings))
        run.begin_resume(checks=[lambda saved: check_micro_batches_per_pass(saved, args.micro_batches_per_pass)],
                         train_batch_size=flag_batch_size, hidden_dropout_prob=p_hidden, attention_probs_dropout_prob=p_attention,
                         extra=fingerprint_extra(args))
        tokenizer = BertTokenizer.from_pretrained(args.bert_model_name)

        # the data first: ClusterDataset reads its folder with a process pool, and nothing forks once the GPU is in use
        # (the samplers draw from `random` / `np.random`, the model's initialisation from torch: the order does not matter)
        eval_dataset = ReDataset(tokenizer, args.predict_file, args.max_query_length, args.max_seq_length)
        if len(eval_dataset) == 0:
            raise ValueError(f"{args.predict_file} holds no example")
        if not os.path.isdir(args.train_file):
            train_dataset = ReDataset(tokenizer, args.train_file, args.max_query_length, args.max_seq_length, args.filter)
            sampler = ReSampler(train_dataset)
        else:
            train_dataset = ClusterDataset(tokenizer, args.train_file, args.max_query_length, args.max_seq_length, args.filter)
            sampler = ClusterSampler(train_dataset, args.train_batch_size)
        if len(train_dataset) == 0:
            raise ValueError(f"{args.train_file} holds no example")
        train_batches = batch_slices(sampler, args.train_batch_size)      # the same order every epoch, as the reference's
        workers = max(0, min(args.eval_workers, usable_cpus() - 2))
        collate = ReTokenizeCollate(tokenizer, args.max_query_length, args.max_seq_length, native_threads=workers)
        train_texts, eval_texts = ReTextView(train_dataset), ReTextView(eval_dataset)

        def tensors(texts, indices):
            batch = collate([texts[i] for i in indices])
            batch.pop("seq_lens_q", None)       # host lists the inference class takes; the module reads the masks
            batch.pop("seq_lens_c", None)
            return batch

        def eval_dataloader():
            n = len(eval_texts)
            return (tensors(eval_texts, range(b0, min(b0 + args.predict_batch_size, n)))
                    for b0 in range(0, n, args.predict_batch_size))
        logger.info(f"Num of dev batches: {-(-len(eval_texts) // args.predict_batch_size)}")

        device = torch.device("cuda", torch.cuda.current_device())
        logger.info("device %s n_gpu %d distributed training %r", device, 1, False)
        model = TrainableRetriever(cfg, device=device, hidden_dropout_prob=p_hidden, attention_probs_dropout_prob=p_attention,
                                   dropout_seed=args.seed, deterministic=args.deterministic)
        if args.deterministic:
            logger.info("--deterministic: the word-embedding gradient is summed in a fixed order (no atomics); a run is a "
                        "function of the data, the seed and the checkpoint, bit for bit")
        if not run.resuming:
            if args.init_checkpoint != "":
                state = torch.load(args.init_checkpoint, map_location="cpu")
            else:
                state = initial_state_dict(cfg, load_bert_weights(args.bert_model_name), args.seed)
            model.load_state_dict(state)
        for n, p in model.named_parameters():
            if any(s in n for s in FROZEN_PARAMETERS):
                p.requires_grad_(False)
        print(f"number of trainable parameters: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")

        optimizer = FusedAdamW(parameter_groups(model, args.weight_decay), lr=args.learning_rate, eps=args.adam_epsilon,
                               max_grad_norm=args.max_grad_norm, loss_scale="dynamic", half_copies=model.half_weights())
        logger.info("activations and their gradients are fp16 with or without --fp16 (fp32 masters, dynamic loss scale); "
                    "--fp16_opt_level is ignored")
        run.tb = tb = tensorboard(tb_dir)
        meter, G, M = run.meter, args.gradient_accumulation_steps, args.micro_batches_per_pass
        passes = []                # [[batch_step of every micro-batch of the pass]] of this run
        if M > 1:
            if G == 1:
                logger.info("--micro-batches-per-pass %d with --gradient_accumulation_steps 1: every micro-batch is followed "
                            "by an update, so every pass holds one micro-batch", M)
            else:
                logger.info("--micro-batches-per-pass %d: up to %d micro-batches of an accumulation window share one pass per "
                            "tower and one block-diagonal loss call; every micro-batch keeps its own in-batch negatives.  "
                            "The run is a function of (data, seed, checkpoint, M), not the M = 1 run bit for bit", M, M)
            torch.cuda.reset_peak_memory_stats(device)
        model.train()
        if run.attach(model, optimizer, len(train_dataset), lambda: [i for b in train_batches for i in b]) is not None:
            if run.stop_training and run.start_position == 0:
                run.start_epoch = int(args.num_train_epochs)        # the straight run left its loop at the end of that epoch
            run.log_resumed("micro-batch")

        logger.info("Start training....")
        run.t_start = time.perf_counter()
        for epoch in range(run.start_epoch, int(args.num_train_epochs)):
            position = run.start_position if epoch == run.start_epoch else 0
            while position < len(train_batches):
                # the pass: consecutive micro-batches up to M, an update step or the end of the epoch (pass_schedule)
                in_pass = []
                while True:
                    run.batch_step += 1
                    in_pass.append(position)
                    position += 1
                    if len(in_pass) >= M or is_update_step(run.batch_step, G) or position == len(train_batches):
                        break
                passes.append(list(range(run.batch_step - len(in_pass) + 1, run.batch_step + 1)))
                position -= 1                                        # of the pass's last micro-batch
                if len(in_pass) == 1:
                    batch = move_to_cuda(tensors(train_texts, train_batches[position]), device)
                    outputs = model(batch)
                    loss = inbatch_loss(outputs["q"], outputs["c"])
                    if G > 1:
                        loss = loss / G
                    optimizer.scale_loss(loss).backward()
                    meter.add(loss.detach(), run.global_step)
                else:
                    # one collate over the pass's examples, one pass per tower, one loss call, one backward
                    sizes = [len(train_batches[p]) for p in in_pass]
                    batch = move_to_cuda(tensors(train_texts, [i for p in in_pass for i in train_batches[p]]), device)
                    rows = [0]
                    for n in sizes:
                        rows.append(rows[-1] + n)
                    outputs = model([{k: v[rows[m]:rows[m + 1]] for k, v in batch.items()} for m in range(len(sizes))])
                    losses = inbatch_loss_blocks(outputs["q"], outputs["c"], outputs["block_sizes"]) / G
                    optimizer.scale_loss(losses.sum()).backward()
                    for loss in losses.detach().unbind(0):
                        meter.add(loss, run.global_step)

                if is_update_step(run.batch_step, G):
                    optimizer.step()      # the unscale, the clip of --max_grad_norm and AdamW, in one fused step
                    model.zero_grad()
                    run.after_update()
                    global_step, wrote_last = run.global_step, False

                    if global_step % args.save_checkpoints_steps == 0:
                        meter.flush(tb)
                        torch.save(model.state_dict(), os.path.join(args.output_dir, f"checkpoint_{global_step}.pt"))

                    if global_step % args.eval_period == 0:
                        meter.flush(tb)
                        acc = predict(args, model, eval_dataloader(), device, fp16=args.efficient_eval)
                        logger.info("Step %d Train loss %.2f Acc %.2f on epoch=%d" % (global_step, meter.avg, acc * 100, epoch))
                        run.evals.append({"step": global_step, "acc": acc, "train_loss_avg": meter.avg})
                        if tb is not None:
                            tb.add_scalar("dev_acc", acc * 100, global_step)
                        # save most recent model
                        torch.save(model.state_dict(), os.path.join(args.output_dir, "checkpoint_last.pt"))
                        best_acc = run.best
                        if run.note_score(acc):
                            logger.info("Saving model with best  Acc %.2f -> Acc %.2f on epoch=%d" % (best_acc * 100, acc * 100, epoch))
                            torch.save(model.state_dict(), os.path.join(args.output_dir, "checkpoint_best.pt"))
                        wrote_last = True

                    if run.save_due(also=wrote_last):
                        # (after an epoch's last micro-batch the next one is the first of the next epoch)
                        nxt = (epoch, position + 1) if position + 1 < len(train_batches) else (epoch + 1, 0)
                        run.save_state(*nxt, True)
                    if run.stopped_early:
                        break
                position += 1
            if run.stop_training or run.stopped_early:
                break
        own = {}
        if M != 1:
            peak = torch.cuda.max_memory_allocated(device)
            logger.info("--micro-batches-per-pass %d: %d passes over %d micro-batches, peak device allocation %.2f GiB", M,
                        len(passes), sum(len(p) for p in passes), peak / 2 ** 30)
            own = dict(micro_batches_per_pass=M, passes=passes, peak_memory_bytes=int(peak))
        return run.finish(LAST_RUN_STATS, best_acc=run.best, **own)


if __name__ == "__main__":
    main()
