"""Command-line flags of the retrieval scripts.

Drop-in for /root/reference/retrieval/config.py:4-93: every flag the reference declares is
accepted with the same spelling (mixed '-' / '_'), type and default, so existing shell scripts
(get_para_embed.sh, README.md:29-37) run unchanged.  Training-only flags are parsed and ignored
by the encode path.  Extra flags of this implementation are listed in EXTRA_FLAGS.
"""
import argparse

# (flag, kind, default) — kind is a type for valued flags or "flag" for store_true switches
_REFERENCE_FLAGS = (
    ("--bert_model_name", str, "bert-large-cased-whole-word-masking"),
    ("--output_dir", str, "logs"),
    ("--weight_decay", float, 0.0),
    ("--load", "flag", False),
    ("--num_workers", int, 5),
    ("--train_file", str, ""),
    ("--predict_file", str, ""),
    ("--init_checkpoint", str, ""),
    ("--max_seq_length", int, 512),
    ("--max_query_length", int, 30),
    ("--do_train", "flag", False),
    ("--do_predict", "flag", False),
    ("--train_batch_size", int, 8),
    ("--predict_batch_size", int, 100),
    ("--learning_rate", float, 5e-5),
    ("--adam_epsilon", float, 1e-8),
    ("--num_train_epochs", float, 5000),
    ("--wait_step", int, 100),
    ("--save_checkpoints_steps", int, 20000),
    ("--iterations_per_loop", int, 1000),
    ("--no_cuda", "flag", False),
    ("--local_rank", int, -1),
    ("--accumulate_gradients", int, 1),
    ("--seed", int, 3),
    ("--gradient_accumulation_steps", int, 1),
    ("--eval-period", int, 2500),
    ("--verbose", "flag", False),
    ("--efficient_eval", "flag", False),
    ("--max_grad_norm", float, 5.0),
    ("--fp16", "flag", False),
    ("--fp16_opt_level", str, "O1"),
    ("--filter", "flag", False),
    ("--prefix", str, "eval"),
    ("--debug", "flag", False),
    ("--eval-workers", int, 32),
    ("--use-whole-model", "flag", False),
    ("--joint-train", "flag", False),
    ("--max-pool", "flag", False),
    ("--shared-norm", "flag", False),
    ("--retriever-path", str, ""),
    ("--qa-drop", float, 0),
    ("--embed_save_path", str, ""),
    ("--is_query_embed", "flag", False),
)

EXTRA_FLAGS = (
    # fp32 .npy output (the reference writes whatever dtype the model emitted: fp16 under --fp16)
    ("--embed_dtype", str, "auto"),
    # pretrain_retriever.py: the word-embedding gradient summed in a fixed order (bit-reproducible training)
    ("--deterministic", "flag", False),
    # pretrain_retriever.py: up to M micro-batches of an accumulation window share one pass per tower and one block-diagonal
    # loss call (every micro-batch keeps its own in-batch negatives); 1 = one pass per micro-batch, the reference's loop
    ("--micro-batches-per-pass", int, 1),
)

# the training commands' checkpoint / resume flags (pretrain_retriever.py and train_reader.py; proqa_amd/checkpoint.py)
STATE_FLAGS = (
    # write trainer_state_last.pt (masters, AdamW moments, counters, sampler and RNG state) every --save_checkpoints_steps
    ("--save-state", "flag", False),
    # stop after this many updates (counted from the run's first, across resumes), state written; implies --save-state
    ("--stop-after-updates", int, 0),
    # continue from a state file, or from a run directory that holds trainer_state_last.pt
    ("--resume", str, ""),
    # every N updates a 64-bit digest of the masters and both moments goes into the stats and the log (0 = never)
    ("--digest-every", int, 0),
)


def add_flags(parser, flags):
    for flag, kind, default in flags:
        if kind == "flag":
            parser.add_argument(flag, action="store_true", default=default)
        else:
            parser.add_argument(flag, type=kind, default=default)
    return parser


def check_state_flags(args, command):
    """the refusals of the checkpoint flags; --stop-after-updates implies --save-state"""
    if args.resume and args.init_checkpoint:
        raise SystemExit(f"{command}: --resume together with --init_checkpoint is refused: the state file carries the weights")
    if args.stop_after_updates < 0:
        raise SystemExit(f"{command}: --stop-after-updates must not be negative")
    if args.digest_every < 0:
        raise SystemExit(f"{command}: --digest-every must not be negative")
    if args.stop_after_updates > 0:
        args.save_state = True
    return args


def build_parser():
    parser = argparse.ArgumentParser()
    return add_flags(parser, _REFERENCE_FLAGS + EXTRA_FLAGS + STATE_FLAGS)


def get_args(argv=None):
    return build_parser().parse_args(argv)
