"""What pretrain_retriever.py and train_reader.py share around their loops: the refusals common to
both, the seeds, the loss meter, and TrainerRun -- the run directory with log.txt and tensorboard, the trainer's counters,
the early-stopping rule, and --save-state / --stop-after-updates / --resume / --digest-every (proqa_amd/checkpoint.py).
The loops, the data, the models and the evaluations are the commands'.  Nothing here has a logger of its own: log.txt
prints %(name)s and its handlers hang on the command's logger, so every line goes through the logger the command passes in.
"""
import json
import logging
import os
import random
import time


def check_train_args(args, command, predict_alone):
    """The refusals both training commands raise, and --do_train implied.  predict_alone: what --do_predict without
    --do_train is and the command that runs it."""
    if args.accumulate_gradients < 1:
        raise ValueError("Invalid accumulate_gradients parameter: {}, should be >= 1".format(args.accumulate_gradients))
    if args.do_predict and not args.do_train:
        raise SystemExit(f"{command}: --do_predict alone is {predict_alone} --do_predict --init_checkpoint ...")
    args.do_train = True
    if not args.train_file:
        raise ValueError("If `do_train` is True, then `train_file` must be specified.")
    if not args.predict_file:
        raise ValueError("If `do_train` is True, then `predict_file` must be specified.")
    if args.local_rank != -1:
        raise SystemExit(f"{command}: --local_rank (DistributedDataParallel) is not supported: one GPU per run")
    if args.no_cuda:
        raise SystemExit(f"{command}: --no_cuda: proqa_amd has no CPU path")
    if args.gradient_accumulation_steps < 1:
        raise ValueError(f"Invalid gradient_accumulation_steps parameter: {args.gradient_accumulation_steps}, should be >= 1")
    return args


def seed_everything(seed):
    import numpy as np
    import torch
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


class Losses:
    """The reference's AverageMeter and its per-batch record without a host read per batch: device scalars queue up and
    are read together at flush()."""

    def __init__(self):
        self.pending, self.pending_steps = [], []
        self.values, self.steps = [], []

    def add(self, loss, global_step):
        self.pending.append(loss)
        self.pending_steps.append(global_step)

    def flush(self, tb=None):
        if self.pending:
            import torch
            new = torch.stack(self.pending).cpu().tolist()
            for value, step in zip(new, self.pending_steps):
                self.values.append(value)
                self.steps.append(step)
                if tb is not None:
                    tb.add_scalar("batch_train_loss", value, step)
                    tb.add_scalar("smoothed_train_loss", sum(self.values) / len(self.values), step)
            self.pending, self.pending_steps = [], []

    @property
    def avg(self):
        return sum(self.values) / len(self.values) if self.values else 0.0


def tensorboard(log_dir):
    try:
        from torch.utils.tensorboard import SummaryWriter
    except Exception:
        return None
    return SummaryWriter(log_dir)


class TrainerRun:
    """One run of a training command: plain state and the steps around the loop that both commands take.

    `with TrainerRun(command, args, logger) as run:` creates args.output_dir and attaches log.txt and the console to
    `logger`; leaving it writes out the last trainer state, closes tensorboard and whatever is in `closing`, and detaches
    the handlers.  Inside: begin_resume() before the data and the model are built, attach() once model and optimizer exist,
    then the command's loop with after_update(), note_score(), save_due() and save_state(), and finish()."""

    def __init__(self, command, args, logger):
        self.command, self.args, self.logger = command, args, logger
        self.global_step = 0      # gradient update step
        self.batch_step = 0       # forward batch count
        self.best, self.wait_step, self.stop_training, self.stopped_early = 0, 0, False, False
        self.evals, self.meter = [], Losses()
        self.start_epoch, self.start_position, self.epoch_started = 0, 0, False
        # checkpoint / resume: nothing of it exists without the four flags
        self.fp = self.ckpt = self.digests = self.state_path = self._saved = None
        self._fp_early = {}
        self.tb, self.closing, self._handlers = None, [], []
        self.model = self.optimizer = None
        self.t_start = time.perf_counter()       # (the command sets it again where its loop begins)

    def __enter__(self):
        out = self.args.output_dir
        if os.path.exists(out) and os.listdir(out):
            print(f"output directory {out} already exists and is not empty.")
        os.makedirs(out, exist_ok=True)
        self._handlers = [logging.FileHandler(os.path.join(out, "log.txt")), logging.StreamHandler()]
        for h in self._handlers:
            h.setFormatter(logging.Formatter("%(asctime)s - %(levelname)s - %(name)s - %(message)s", datefmt="%m/%d/%Y %H:%M:%S"))
            self.logger.addHandler(h)
        self.logger.setLevel(logging.INFO)
        self.logger.propagate = False
        return self

    def __exit__(self, *exc):
        if self.ckpt is not None:
            try:
                self.ckpt.close()
            except Exception:
                self.logger.exception("the last trainer state was not written")
        for c in [self.tb] + self.closing:
            if c is not None:
                c.close()
        for h in self._handlers:
            self.logger.removeHandler(h)
            h.close()
        self._handlers = []

    # -- resume ------------------------------------------------------------------------------------------------------------
    def _fingerprint(self, **late):
        from . import checkpoint
        return checkpoint.fingerprint(self.command, self.args, **self._fp_early, **late)

    def begin_resume(self, checks=(), **early):
        """The flags first: with --resume a run of other settings is refused before the data and the model are built.
        early: checkpoint.fingerprint()'s keywords that are known by now; checks: the command's own, called on the saved
        fingerprint before the fields are compared."""
        self._fp_early = early
        self.fp = self._fingerprint()
        if self.args.resume:
            from . import checkpoint
            self._saved = checkpoint.read_state(checkpoint.resolve_state_path(self.args.resume))
            for check in checks:
                check(self._saved["trainer"]["fingerprint"])
            checkpoint.check_fingerprint(self._saved["trainer"]["fingerprint"], self.fp, fields=tuple(self.fp))

    @property
    def resuming(self):
        return self._saved is not None

    def attach(self, model, optimizer, n_train, order):
        """Model and optimizer exist.  With one of the four flags: the full fingerprint (order: a callable, it can be long),
        the checkpoint writer and the digest log; with --resume the state file goes into model, optimizer, the RNGs and the
        counters, and its "trainer" entry is returned (else None) for what the command keeps there.  The command then sets
        start_epoch for a run that had stopped and calls log_resumed()."""
        from . import checkpoint
        args, saved, self._saved = self.args, self._saved, None       # (the file's flat buffer is not kept)
        self.model, self.optimizer = model, optimizer
        self.state_path = os.path.join(args.output_dir, checkpoint.STATE_FILE)
        if not (args.save_state or args.digest_every > 0 or saved is not None):
            return None
        self.fp = self._fingerprint(n_train=n_train, order=order(), model=model)
        if saved is not None:
            checkpoint.check_fingerprint(saved["trainer"]["fingerprint"], self.fp)
        self.ckpt = checkpoint.TrainerCheckpoint(model, optimizer)
        self.digests = checkpoint.DigestLog(self.ckpt, args.digest_every)
        if saved is None:
            return None
        tr = self.ckpt.load(saved)
        checkpoint.set_rng_states(tr["rng"])
        self.global_step, self.batch_step, self.best = tr["global_step"], tr["batch_step"], tr["best"]
        self.wait_step, self.stop_training, self.evals = tr["wait_step"], tr["stop_training"], list(tr["evals"])
        self.meter.values, self.meter.steps = list(tr["losses"]), list(tr["loss_steps"])
        self.digests.entries = [dict(e) for e in tr["state_digests"]]
        self.start_epoch, self.start_position, self.epoch_started = tr["epoch"], tr["position"], tr["epoch_started"]
        if 0 < args.stop_after_updates <= self.global_step:
            raise SystemExit(f"{self.command}: --stop-after-updates {args.stop_after_updates}: the state file already "
                             f"holds {self.global_step} updates")
        return tr

    def log_resumed(self, unit):
        """unit: what batch_step counts ("micro-batch", "question")"""
        self.logger.info("Resumed from %s: update %d, %s %d, epoch %d position %d.  %s", self.args.resume, self.global_step,
                         unit, self.batch_step, self.start_epoch, self.start_position,
                         "With --deterministic the run continues bit for bit as the uninterrupted one."
                         if self.args.deterministic else
                         "Without --deterministic the word-embedding gradient's atomics make two runs differ, resumed or not.")

    # -- the loop ----------------------------------------------------------------------------------------------------------
    def after_update(self):
        self.global_step += 1
        if self.digests is not None:
            self.digests.after_update(self.global_step)

    def note_score(self, score, patience=True):
        """The early-stopping rule after an evaluation; True when `score` is a new best (the command then saves its model).
        patience=False is the reader's end-of-epoch evaluation, the reference's: a score that is no better does not count
        towards --wait_step, and a better one does not take stop_training back."""
        if self.best < score:
            self.best, self.wait_step = score, 0
            if patience:
                self.stop_training = False
            return True
        if patience:
            self.wait_step += 1
            if self.wait_step == self.args.wait_step:
                self.stop_training = True
        return False

    def save_due(self, also=False):
        """After an update: whether the trainer state is written now (every --save_checkpoints_steps updates, at
        --stop-after-updates, or when the command says `also`).  Sets stopped_early: the command leaves its loops."""
        if not self.args.save_state:
            return False
        self.stopped_early = self.global_step == self.args.stop_after_updates
        return self.global_step % self.args.save_checkpoints_steps == 0 or also or self.stopped_early

    def save_state(self, epoch, position, epoch_started, **sections):
        """The trainer state as of now, written behind the training stream (the losses are read here: allowed).  The next
        micro-batch is number `position` of `epoch`; sections: the command's own (reader=...)."""
        from . import checkpoint
        self.meter.flush(self.tb)
        self.digests.flush(self.logger)
        self.ckpt.snapshot(self.state_path, dict(checkpoint.trainer_state(
            fingerprint=self.fp, global_step=self.global_step, batch_step=self.batch_step, epoch=epoch, position=position,
            epoch_started=epoch_started, best=self.best, wait_step=self.wait_step, stop_training=self.stop_training,
            dropout=checkpoint.dropout_states(self.model), losses=self.meter.values, loss_steps=self.meter.steps,
            evals=self.evals,
            param_groups=[{"lr": g["lr"], "weight_decay": g["weight_decay"]} for g in self.optimizer.param_groups],
            state_digests=self.digests.entries, **sections), rng=checkpoint.rng_states()))

    def finish(self, stats, **own):
        """The loop is over: the last reads, the last state written out, and the run's figures put into the command's
        `stats` dict (in place) with the command's `own`, then into the file PROQA_STATS_JSON names."""
        self.meter.flush(self.tb)
        if self.ckpt is not None:
            self.digests.flush(self.logger)
            self.ckpt.close()
        fused = self.optimizer.state_dict()["fused"]
        seconds = time.perf_counter() - self.t_start
        self.logger.info("Training finished!")
        stats.clear()
        stats.update(global_step=self.global_step, batch_steps=self.batch_step, losses=self.meter.values, evals=self.evals,
                     skipped_steps=fused["skipped_steps"], loss_scale=fused["loss_scale"], seconds=seconds,
                     output_dir=self.args.output_dir, deterministic=bool(self.args.deterministic), **own)
        if self.args.stop_after_updates > 0:
            stats["stopped_early"] = self.stopped_early
        if self.args.digest_every > 0:
            stats["state_digests"] = self.digests.entries
        if os.environ.get("PROQA_STATS_JSON"):
            with open(os.environ["PROQA_STATS_JSON"], "w") as f:
                json.dump(stats, f)
        return stats
