"""`python train_reader.py --raw-train-data train.txt --raw-eval-data dev.txt --matched-para-path matched.txt ...`: reader
training, the --do_train loop of qa/train_retrieve_qa.py:170-265 on one MI355X.

Same flags (qa/config.py, plus --index2paraid as predict_qa has it), same output directory, model_name and log.txt, the
same seeds, accumulation rule (batch_step counts a failed retrieval, which therefore uses up an update slot), the
per-epoch `Failed retrieval: x/N` line, evaluation every --eval_period updates and after every epoch, best-model.pt,
model-{epoch+1}-{em}.pt after epoch 16, wait_step / stop_training.  The model is TrainableReader with the config's two
dropout rates, the optimizer FusedAdamW with the reference's two parameter groups, a dynamic loss scale and the clip of
--max_grad_norm inside the fused step; the batches come from proqa_amd.online_sampler.OnlineSampler, whose per-question
retrieval stays on the device.

Intended differences: the sampler's (its question pass in eval(), the exact search, sorted matched
strings); activations are fp16 with or without --fp16 and --fp16_opt_level is ignored; the host never reads a loss inside
the loop (they are read at an evaluation, at the end of an epoch and at the end); the dev evaluation is predict_qa.evaluate
-- all questions at once over the BertReader that TrainableReader builds for eval(), on the SAME IndexFlatIP the sampler
searches (the model is back in train() after it, as after the reference's predict()); the initial weights come from --init_checkpoint, or from the local
--bert_model_name directory plus --retriever-path (nothing is fetched); --do_predict alone, --local_rank, --no_cuda,
--use-spanbert, --separate and --add-select are refused.  `train_retrieve_qa.py` keeps its refusal of the training flags.

Beyond the reference (proqa_amd/checkpoint.py): --save-state, --stop-after-updates, --resume and
--digest-every as in pretrain_retriever.py; the state also holds the sampler's permutation, the failed and update steps
and the RNG states, so a run resumed inside an epoch visits the questions the uninterrupted run visits.
--questions-per-pass Q (default 1): within an accumulation window no weight changes, so up to Q of its questions are drawn
from the sampler one after another and then run through ONE forward (TrainableReader on the list: one pass per tower, one
fused loss call) and one backward; pass_schedule() is the grouping rule, and Q = 1, the reference's loop, is its smallest
case.  The optimisation step is the one of the questions run one after another; with --gradient_accumulation_steps 1 every
pass holds one question.
--sampler-lookahead W (default 1): the sampler retrieves up to W questions in one sampling step -- one question-tower pass, one
search, one collect launch, one record copy (OnlineSampler.retrieve_many) -- never past the next update slot, so every
question is retrieved with the weights its own retrieval would have read; retrieval_groups() is the grouping rule, and W = 1
is today's loop, untouched.  A tower pass over W questions need not give the fp16 bits of W passes over one, so a run with
W > 1 is a function of (data, seed, checkpoint, W), not the W = 1 run's bits.
"""
import argparse
import dataclasses
import json
import logging
import os
import time

from .pretrain_retriever import is_update_step, load_bert_weights, load_model_config, parameter_groups
from .trainer import TrainerRun, check_train_args, seed_everything, tensorboard

LAST_RUN_STATS = {}

# test hooks: parameters whose name contains one of these substrings are frozen (without --deterministic the word-embedding
# gradient is summed with atomics, the module's one run-to-run difference); a callable that receives every non-empty batch
# before the forward; False = per-forward casts in the retriever's towers instead of the fp16 working copies
FROZEN_PARAMETERS = ()
ON_BATCH = None
USE_HALF_COPIES = True

logger = logging.getLogger(__name__)


# ---- pure pieces (no GPU) ------------------------------------------------------------------------------------------------

def build_parser():
    """the flags of qa/config.py, plus --index2paraid"""
    p = argparse.ArgumentParser(description="ProQA reader training (qa/train_retrieve_qa.py --do_train) on MI355X")
    p.add_argument("--bert_model_name", default="bert-base-uncased", type=str)
    p.add_argument("--output_dir", default="logs", type=str)
    p.add_argument("--weight_decay", default=0.0, type=float)
    p.add_argument("--load", default=False, action="store_true")
    p.add_argument("--num_workers", default=5, type=int)
    p.add_argument("--train_file", type=str, default="../../data/mrqa-train/HotpotQA-tokenized.jsonl")
    p.add_argument("--predict_file", type=str, default="../../data/mrqa-dev/HotpotQA-tokenized.jsonl")
    p.add_argument("--init_checkpoint", type=str, default="")
    p.add_argument("--do_lower_case", default=True, action="store_true")
    p.add_argument("--max_seq_length", default=512, type=int)
    p.add_argument("--max_query_length", default=50, type=int)
    p.add_argument("--do_train", default=False, action="store_true")
    p.add_argument("--do_predict", default=False, action="store_true")
    p.add_argument("--train_batch_size", default=8, type=int)
    p.add_argument("--predict_batch_size", default=100, type=int)
    p.add_argument("--learning_rate", default=5e-5, type=float)
    p.add_argument("--adam_epsilon", default=1e-8, type=float)
    p.add_argument("--num_train_epochs", default=200, type=float)
    p.add_argument("--wait_step", type=int, default=100)
    p.add_argument("--save_checkpoints_steps", default=1000, type=int)
    p.add_argument("--iterations_per_loop", default=1000, type=int)
    p.add_argument("--no_cuda", default=False, action="store_true")
    p.add_argument("--local_rank", type=int, default=-1)
    p.add_argument("--accumulate_gradients", type=int, default=1)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--eval_period", type=int, default=1000, help="setting to -1: eval only after each epoch")
    p.add_argument("--verbose", action="store_true", default=False)
    p.add_argument("--efficient_eval", action="store_true", help="accepted: the evaluation always runs the fp16 reader")
    p.add_argument("--max_answer_len", default=20, type=int)
    p.add_argument("--max_grad_norm", default=5.0, type=float)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--fp16_opt_level", type=str, default="O1", help="ignored")
    p.add_argument("--qa-drop", default=0, type=float)
    p.add_argument("--rank-drop", default=0, type=float)
    p.add_argument("--MI", action="store_true")
    p.add_argument("--mi-k", default=10, type=int)
    p.add_argument("--max-pool", action="store_true")
    p.add_argument("--eval-workers", default=16, type=int, help="threads of the native WordPiece tokenizer")
    p.add_argument("--save-pred", action="store_true")
    p.add_argument("--retriever-path", type=str, default="")
    p.add_argument("--raw-train-data", type=str, default="../data/nq-train.txt")
    p.add_argument("--raw-eval-data", type=str, default="../data/nq-dev.txt")
    p.add_argument("--fix-para-encoder", action="store_true")
    p.add_argument("--db-path", type=str, default="../data/nq_paras.db")
    p.add_argument("--index-path", type=str, default="retrieval/index_data/para_embed_100k.npy")
    p.add_argument("--index2paraid", type=str, default="retrieval/index_data/idx_id.json",
                   help="idx_id.json of the index (the reference's OnlineSampler default)")
    p.add_argument("--matched-para-path", type=str, default="../data/wq_ft_train_matched.txt")
    p.add_argument("--use-spanbert", action="store_true")
    p.add_argument("--spanbert-path", default="../data/span_bert", type=str)
    p.add_argument("--eval-k", default=5, type=int)
    p.add_argument("--regex", action="store_true")
    p.add_argument("--separate", action="store_true")
    p.add_argument("--add-select", action="store_true")
    p.add_argument("--drop-early", action="store_true")
    p.add_argument("--shared-norm", action="store_true")
    p.add_argument("--prefix", type=str, default="eval")
    p.add_argument("--debug", action="store_true")
    p.add_argument("--use-top-passage", action="store_true")
    p.add_argument("--topk", default=30, type=int)
    p.add_argument("--save-all", action="store_true")
    p.add_argument("--candidates", default="", type=str)
    p.add_argument("--deterministic", action="store_true", default=False,
                   help="sum the word-embedding gradients in a fixed order: a run reproduces bit for bit")
    p.add_argument("--questions-per-pass", default=1, type=int,
                   help="questions of one accumulation window that share a tower pass and one fused loss call (1: one question "
                        "per pass); the optimisation step is the same, so it only pays with --gradient_accumulation_steps > 1")
    p.add_argument("--sampler-lookahead", default=1, type=int,
                   help="questions the sampler retrieves in one sampling step (one tower pass, one search, one collect); a "
                        "group never crosses an update slot, so it only pays with --gradient_accumulation_steps > 1")
    from .config import STATE_FLAGS, add_flags
    return add_flags(p, STATE_FLAGS)       # --save-state, --stop-after-updates, --resume, --digest-every


def get_args(argv=None):
    return build_parser().parse_args(argv)


def model_name(args):
    """the reference's run name (train_retrieve_qa.py:48), from the flags BEFORE train_batch_size is divided"""
    return (f"dense-seed{args.seed}-bsz{args.train_batch_size}-fp16{args.fp16}-{args.prefix}-lr{args.learning_rate}-"
            f"{args.bert_model_name}-qdrop{args.qa_drop}-sn{args.shared_norm}-sep{args.separate}-as{args.add_select}-"
            f"noearly{args.drop_early}")


def check_args(args):
    """The refusals, and --do_train implied.  Raises what the reference raises where it raises."""
    from .online_sampler import MAX_HEAD
    check_train_args(args, "train_reader.py", "the evaluation of a checkpoint: run train_retrieve_qa.py")
    if args.use_spanbert:
        raise SystemExit("train_reader.py: --use-spanbert (a cased reader beside the uncased retriever) is not built")
    if args.separate or args.add_select:
        raise SystemExit("train_reader.py: --separate / --add-select are not built: they need a select term in the loss "
                         "kernels (DESIGN.md section 3h)")
    if args.questions_per_pass < 1:
        raise ValueError(f"Invalid questions_per_pass parameter: {args.questions_per_pass}, should be >= 1")
    if args.sampler_lookahead < 1:
        raise ValueError(f"Invalid sampler_lookahead parameter: {args.sampler_lookahead}, should be >= 1")
    per_question = int(args.train_batch_size / args.accumulate_gradients)
    if not 1 <= per_question <= MAX_HEAD:
        raise ValueError(f"--train_batch_size {args.train_batch_size} / --accumulate_gradients {args.accumulate_gradients}: "
                         f"the passages per question must be in [1, {MAX_HEAD}]")
    if args.matched_para_path == "":
        raise ValueError("--matched-para-path is required: the sampler's labels come from it")
    from .config import check_state_flags
    return check_state_flags(args, "train_reader.py")


def update_schedule(n_batches, gradient_accumulation_steps, failed=()):
    """[batch_step of every optimizer step] over n_batches questions, batch_step counted from 1 across epochs;
    `failed`: the batch steps whose retrieval failed ({}).  batch_step is incremented BEFORE the empty-batch `continue`
    (train_retrieve_qa.py:185-188), so a failed retrieval uses up its slot of (batch_step + 1) % G == 0 and the update of
    that slot does not happen: the gradients go on accumulating until the next slot."""
    failed = set(failed)
    return [b for b in range(1, n_batches + 1) if b not in failed and is_update_step(b, gradient_accumulation_steps)]


def closes_pass(n_in_pass, batch_step, gradient_accumulation_steps, questions_per_pass):
    """Whether the pass is run now, asked when the question of `batch_step` (retrieved, not failed) has just joined it as its
    n_in_pass-th: it is full, or the question sits in an update slot -- the optimizer step needs every gradient of its
    window, and the next question is retrieved with the new weights."""
    return n_in_pass >= questions_per_pass or is_update_step(batch_step, gradient_accumulation_steps)


def pass_schedule(n_batches, gradient_accumulation_steps, questions_per_pass, failed=(), first=1):
    """[[batch_step of every question of the pass]] over ONE epoch of n_batches questions whose batch steps are first ..
    first + n_batches - 1; `failed` as update_schedule.  A failed retrieval joins no pass and closes none: in an update slot it
    leaves the window open, and the pass with it.  What is open when the epoch ends is run as the epoch's last pass (the
    evaluation that follows reads the weights, not the gradients; the window stays open into the next epoch)."""
    failed = set(failed)
    passes, open_pass = [], []
    for b in range(first, first + n_batches):
        if b in failed:
            continue
        open_pass.append(b)
        if closes_pass(len(open_pass), b, gradient_accumulation_steps, questions_per_pass):
            passes.append(open_pass)
            open_pass = []
    if open_pass:
        passes.append(open_pass)
    return passes


def group_length(next_step, gradient_accumulation_steps, lookahead):
    """How many questions, counting the one of batch step `next_step`, can be retrieved together: up to the first update
    slot (the weights can change there), at most `lookahead`.  (The sampler cuts it to what the epoch still holds.)"""
    n = 1
    while n < lookahead and not is_update_step(next_step + n - 1, gradient_accumulation_steps):
        n += 1
    return n


def retrieval_groups(n_batches, gradient_accumulation_steps, lookahead, first=1):
    """[[batch_step of every question of the group]] over ONE epoch of n_batches questions whose batch steps are first ..
    first + n_batches - 1: the questions the sampler retrieves in one sampling step.  A group is a run of consecutive batch
    steps that ends at the first update slot, after `lookahead` steps or with the epoch.  Failed retrievals do not move the
    groups: batch_step counts them, and a failed update slot only means that the weights did not change there, so the cut is
    merely early."""
    groups, b, end = [], first, first + n_batches
    while b < end:
        n = min(group_length(b, gradient_accumulation_steps, lookahead), end - b)
        groups.append(list(range(b, b + n)))
        b += n
    return groups


def reader_fingerprint_extra(args):
    """The reader command's own fields of the resume fingerprint.  questions_per_pass and sampler_lookahead are fields only
    when they are not 1, so that the state files of one-question passes and one-question sampling keep their fingerprint."""
    extra = {"qa_drop": float(args.qa_drop), "shared_norm": bool(args.shared_norm), "drop_early": bool(args.drop_early),
             "fix_para_encoder": bool(args.fix_para_encoder)}
    if int(getattr(args, "questions_per_pass", 1)) != 1:
        extra["questions_per_pass"] = int(args.questions_per_pass)
    if int(getattr(args, "sampler_lookahead", 1)) != 1:
        extra["sampler_lookahead"] = int(args.sampler_lookahead)
    return extra


def check_field_default_1(saved_fingerprint, field, value):
    """SystemExit when the state file was written at another --questions-per-pass or --sampler-lookahead (`field`: a state
    file without the field was written at 1, where check_fingerprint would pass over the field)."""
    was = int(saved_fingerprint.get(field, 1))
    if was != int(value):
        raise SystemExit(f"--resume: the state file was written by a different run: field {field!r} is "
                         f"{int(value)!r} now, was {was!r} when the state was saved")


def initial_state_dict(cfg, bert_weights):
    """{`bert.*`: the pre-trained BertModel} of the reference's untrained BertRetrieveQA; qa_outputs keeps the module's
    own initialisation and the retriever comes from --retriever-path"""
    import torch
    from .retriever import tower_keys
    sd = {}
    for key in tower_keys("bert", cfg.num_hidden_layers):
        bare = key[len("bert."):]
        if bare not in bert_weights:
            raise SystemExit(f"train_reader.py: the BERT weights lack {bare!r}")
        sd[key] = bert_weights[bare].detach().to(torch.float32).clone()
    return sd


# ---- the command -------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class _ReaderCounts:
    """the command's counters beside TrainerRun's: what the "reader" section of a trainer state holds, and pending_grad"""
    passes: int = 0
    pending_grad: bool = False      # a backward has run since the last optimizer step
    groups_before: int = 0          # sampling steps of the run this one resumes
    resumed_failed: int = 0         # failed retrievals of the epoch this run resumes in
    failed_per_epoch: list = dataclasses.field(default_factory=list)
    failed_steps: list = dataclasses.field(default_factory=list)
    update_steps: list = dataclasses.field(default_factory=list)


def main(argv=None):
    args = check_args(get_args(argv))
    import torch
    import zlib
    from transformers import BertTokenizer
    from . import predict_qa
    from .index import IndexFlatIP
    from .online_sampler import OnlineSampler
    from .optim import FusedAdamW
    from .trainable_reader import TrainableReader
    from .utils import DocDB

    name = model_name(args)
    tb_dir = os.path.join(args.output_dir, "tflogs", "dense", name)
    args.output_dir = os.path.join(args.output_dir, name)
    with TrainerRun("train_reader.py", args, logger) as run:
        logger.info(args)
        if not torch.cuda.is_available():
            raise RuntimeError("no MI355X visible: reader training has no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
        logger.info("device %s n_gpu %d distributed training %r", device, 1, False)
        flag_batch_size = args.train_batch_size
        args.train_batch_size = int(args.train_batch_size / args.accumulate_gradients)     # passages per question
        seed_everything(args.seed)

        cfg, p_hidden, p_attention = load_model_config(args.bert_model_name)
        run.begin_resume(checks=[lambda saved: check_field_default_1(saved, "questions_per_pass", args.questions_per_pass),
                                 lambda saved: check_field_default_1(saved, "sampler_lookahead", args.sampler_lookahead)],
                         train_batch_size=flag_batch_size, hidden_dropout_prob=p_hidden,
                         attention_probs_dropout_prob=p_attention, extra=reader_fingerprint_extra(args))
        tokenizer = BertTokenizer.from_pretrained(args.bert_model_name)
        logger.info("Loading para db and pretrained index ...")
        para_db = DocDB(args.db_path)
        run.closing.append(para_db)
        if args.max_seq_length > cfg.max_position_embeddings:
            raise ValueError("Cannot use sequence length %d because the BERT model was only trained up to sequence length %d"
                             % (args.max_seq_length, cfg.max_position_embeddings))
        # ONE copy of the rows in HBM: the sampler searches it and the dev evaluation searches it
        index = IndexFlatIP(128)
        index.add_npy(args.index_path)
        with open(args.index2paraid) as f:
            index2paraid = json.load(f)
        eval_data = predict_qa.load_qa(args.raw_eval_data)

        state = None
        retriever_path = args.retriever_path
        if run.resuming or args.init_checkpoint != "":
            args.retriever_path = ""       # the state file carries every master, the checkpoint the retriever
        else:
            state = initial_state_dict(cfg, load_bert_weights(args.bert_model_name))
        model = TrainableReader.from_args(cfg, args, device, hidden_dropout_prob=p_hidden,
                                          attention_probs_dropout_prob=p_attention, dropout_seed=args.seed)
        args.retriever_path = retriever_path
        if args.init_checkpoint != "":
            model.load_state_dict(torch.load(args.init_checkpoint, map_location="cpu"))
        elif state is not None:
            model.load_state_dict(state, strict=False)
        logger.info(f"number of trainable parameters: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")
        if args.deterministic:
            logger.info("--deterministic: the word-embedding gradient is summed in a fixed order (no atomics); a run is a "
                        "function of the data, the seed and the checkpoint, bit for bit")
        if args.fix_para_encoder:
            model.freeze_c_encoder()
        for n, p in model.named_parameters():
            if any(s in n for s in FROZEN_PARAMETERS):
                p.requires_grad_(False)

        groups = parameter_groups(model, args.weight_decay)
        half_copies = None
        if USE_HALF_COPIES:
            # fp16 working copies of the retriever's matrices (the sampler's question pass reads them); the step writes
            # the copies of the parameters it owns, the frozen passage tower's are cast once and never go stale
            owned = {id(p) for g in groups for p in g["params"]}
            half_copies = {p: h for p, h in model.retriever.half_weights().items() if id(p) in owned}
        optimizer = FusedAdamW(groups, lr=args.learning_rate, eps=args.adam_epsilon, max_grad_norm=args.max_grad_norm,
                               loss_scale="dynamic", half_copies=half_copies)
        logger.info("activations and their gradients are fp16 with or without --fp16 (fp32 masters, dynamic loss scale); "
                    "--fp16_opt_level is ignored")
        run.tb = tb = tensorboard(tb_dir)
        meter, counts = run.meter, _ReaderCounts()

        def evaluate():
            """the dev EM of the current weights: BertReader over an fp16 copy of them, on the sampler's index"""
            meter.flush(tb)
            model.eval()
            try:
                em = predict_qa.evaluate(args, model.inference_reader(), tokenizer, eval_data, index, index2paraid)
            finally:
                model.train()       # (the copy is dropped: the next evaluation takes the weights of its own time)
            return float(em)

        args.search, args.reader_batch = "exact", 256        # what predict_qa.evaluate reads beside the shared flags
        G, Q, W = args.gradient_accumulation_steps, args.questions_per_pass, args.sampler_lookahead
        if Q > 1:
            logger.info("--questions-per-pass %d: the questions of an accumulation window share tower passes and one fused "
                        "loss call%s", Q, "" if G > 1 else "; with --gradient_accumulation_steps 1 every question closes its "
                        "window, so every pass holds one question")
        if W > 1:
            logger.info("--sampler-lookahead %d: the sampler retrieves the questions up to the next update slot, at most %d, in "
                        "one sampling step%s", W, W, "" if G > 1 else "; with --gradient_accumulation_steps 1 every question "
                        "sits in an update slot, so every group holds one question")
        logger.info("Start training....")
        model.train()
        train_dataloader = OnlineSampler(args.raw_train_data, tokenizer, args.max_query_length, args.max_seq_length, para_db,
                                         index, index2paraid=index2paraid, matched_para_path=args.matched_para_path,
                                         regex=args.regex, device=device)

        tr = run.attach(model, optimizer, len(train_dataloader),
                        lambda: [zlib.crc32(qa["question"].encode("utf-8")) for qa in train_dataloader.qa_data])
        if tr is not None:
            saved = tr["reader"]
            train_dataloader.set_permutation(saved["permutation"])      # (shuffle() draws from `random` every epoch)
            counts = _ReaderCounts(passes=int(saved.get("passes", 0)), groups_before=int(saved.get("sampler_groups", 0)),
                                   resumed_failed=saved["failed_retrieval"], failed_per_epoch=list(saved["failed_per_epoch"]),
                                   failed_steps=list(saved["failed_steps"]), update_steps=list(saved["update_steps"]))
            if run.stop_training and not run.epoch_started:
                run.start_epoch = int(args.num_train_epochs)        # the straight run left its loop at the end of that epoch
            run.log_resumed("question")

        def save_state(next_epoch, next_position, started, failed_so_far):
            reader_state = {"failed_steps": list(counts.failed_steps), "update_steps": list(counts.update_steps),
                            "failed_per_epoch": list(counts.failed_per_epoch), "failed_retrieval": int(failed_so_far),
                            "permutation": train_dataloader.permutation()}
            if Q != 1:
                reader_state["passes"] = int(counts.passes)
            if W != 1:
                reader_state["sampler_groups"] = counts.groups_before + train_dataloader.groups
            run.save_state(next_epoch, next_position, started, reader=reader_state)

        def run_pass(batches):
            """forward + backward of the questions of one pass: one forward on the list; every question's loss is divided
            by G and their sum goes through the loss scale"""
            for b in batches:
                if ON_BATCH is not None:
                    ON_BATCH(b)
            losses = model([b["net_input"] for b in batches])["losses"]
            if G > 1:
                losses = losses / G
            optimizer.scale_loss(losses.sum()).backward()
            for i in range(len(batches)):
                meter.add(losses[i].detach(), run.global_step)
            counts.passes += 1
            counts.pending_grad = True

        run.t_start = time.perf_counter()
        for epoch in range(run.start_epoch, int(args.num_train_epochs)):
            resumed_here = run.epoch_started and epoch == run.start_epoch       # inside a saved epoch: its shuffle is in the state
            if not resumed_here:
                train_dataloader.shuffle()
            failed_retrieval = counts.resumed_failed if resumed_here else 0
            position = run.start_position if resumed_here else 0
            open_pass = []
            load_args = {"start": position} if position else {}
            if W != 1:
                # asked when the sampler has handed out all it retrieved: batch_step + 1 is the step of its next question
                load_args["lookahead"] = lambda: group_length(run.batch_step + 1, G, W)
            for batch in train_dataloader.load(model.retriever, k=args.train_batch_size, **load_args):
                run.batch_step += 1
                position += 1
                if batch == {}:
                    failed_retrieval += 1
                    counts.failed_steps.append(run.batch_step)
                    continue
                open_pass.append(batch)
                if not closes_pass(len(open_pass), run.batch_step, G, Q):
                    continue
                run_pass(open_pass)
                open_pass = []

                if is_update_step(run.batch_step, G):
                    optimizer.step()      # the unscale, the clip of --max_grad_norm and AdamW, in one fused step
                    model.zero_grad()
                    run.after_update()
                    global_step = run.global_step
                    counts.update_steps.append(run.batch_step)
                    counts.pending_grad = False

                    if args.eval_period != -1 and global_step % args.eval_period == 0:
                        em = evaluate()
                        logger.info("Step %d Train loss %.2f EM %.2f on epoch=%d" % (global_step, meter.avg, em * 100, epoch))
                        run.evals.append({"step": global_step, "epoch": epoch, "em": em, "train_loss_avg": meter.avg})
                        if tb is not None:
                            tb.add_scalar("dev_em", em * 100, global_step)
                        best_em = run.best
                        if run.note_score(em):
                            logger.info("Saving model with best EM: %.2f -> EM %.2f on epoch=%d" % (best_em * 100, em * 100, epoch))
                            torch.save({k: v.cpu() for k, v in model.state_dict().items()},
                                       os.path.join(args.output_dir, "best-model.pt"))

                    if run.save_due():
                        save_state(epoch, position, True, failed_retrieval)
                    if run.stopped_early:
                        break
            if run.stopped_early:
                break
            if open_pass:       # the epoch ended inside a window: its last questions are a pass of their own
                run_pass(open_pass)

            logger.info(f"Failed retrieval: {failed_retrieval}/{len(train_dataloader)} ...")
            counts.failed_per_epoch.append(failed_retrieval)
            em = evaluate()
            run.evals.append({"step": run.global_step, "epoch": epoch, "em": em, "train_loss_avg": meter.avg,
                              "end_of_epoch": True})
            if tb is not None:
                tb.add_scalar("dev_em", em * 100, run.global_step)
            logger.info(f"average training loss {meter.avg}")
            best_em = run.best
            if run.note_score(em, patience=False):      # (the reference's rule here: no wait_step count, no stop taken back)
                logger.info("Saving model with best EM: %.2f  -> %.2f on epoch=%d" % (best_em * 100, em * 100, epoch))
                torch.save(model.state_dict(), os.path.join(args.output_dir, "best-model.pt"))
            if epoch > 15:
                logger.info(f"Saving model after epoch {epoch + 1}")
                torch.save(model.state_dict(), os.path.join(args.output_dir, f"model-{epoch+1}-{em}.pt"))
            if args.save_state:
                if counts.pending_grad:
                    logger.info("no trainer state at the end of epoch %d: a gradient is accumulated and waits for its update", epoch)
                else:
                    save_state(epoch + 1, 0, False, 0)
            if run.stop_training:
                break
        own = dict(failed_retrieval=counts.failed_per_epoch, failed_steps=counts.failed_steps, update_steps=counts.update_steps,
                   best_em=run.best, sampler_seconds=dict(train_dataloader.seconds),
                   sampler_transfers=dict(train_dataloader.transfers), questions_per_pass=Q, passes=counts.passes)
        if W != 1:
            own.update(sampler_lookahead=W, sampler_groups=counts.groups_before + train_dataloader.groups)
        return run.finish(LAST_RUN_STATS, **own)


if __name__ == "__main__":
    main()
