"""Trainer state on disk: what `--save-state`, `--stop-after-updates`, `--resume` and `--digest-every` of the two training
commands are built on.

    StateSnapshotter(tensors)   one flat device buffer and one pinned host buffer of the same layout.  snapshot(path, meta)
                                enqueues proqa_state_snapshot (copy + one 64-bit digest per tensor, two launches) on torch's
                                current stream and returns without waiting for the device; a side stream copies the flat
                                buffer and the digests to pinned memory, a writer thread serialises them to `path`.tmp,
                                fsyncs and renames.  digest() is the digest-only call.
    TrainerCheckpoint(model, optimizer)
                                the snapshotter over the fp32 masters, exp_avg, exp_avg_sq and the optimizer's device
                                scalars; snapshot(path, trainer) writes one self-contained file, load(path) puts it back,
                                recomputes the digests on the device and compares them with the file's.
    trainer_state / fingerprint / check_fingerprint
                                everything beyond the tensors that determines the rest of a run, and what must not change
                                between the two halves of one.

A state file is a torch.save of plain containers, numbers, strings and tensors (it loads with weights_only=True):
{"format", "names", "shapes", "numel", "offsets", "flat" (uint8, the snapshot buffer: tensor t's fp32 words at offsets[t],
256-byte aligned), "digests" (int64: the uint64 digests' bits), "trainer"}.
"""
import hashlib
import os
import random
import threading
import time

import numpy as np
import torch

from . import _lib

FORMAT = 1
STATE_FILE = "trainer_state_last.pt"
DEVICE_STATE = "optimizer.device_state"      # FusedAdamW's 64 bytes of device scalars, as 16 fp32 words
_MASK64 = (1 << 64) - 1


# ---- pure pieces (no GPU) ------------------------------------------------------------------------------------------------

def layout(numels, align=_lib.STATE_DST_ALIGN):
    """(byte offsets of the tensors in the flat buffer, its size): every tensor starts on an `align`-byte boundary"""
    offsets, at = [], 0
    for n in numels:
        offsets.append(at)
        at += -(-(int(n) * 4) // align) * align
    return offsets, at


def combine_digests(digests):
    """One 64-bit number from per-tensor digests in their order: h = h * 0x100000001B3 + d mod 2^64, from h = 0 (order
    sensitive, so two tensors that trade places change it)."""
    h = 0
    for d in digests:
        h = (h * 0x100000001B3 + (int(d) & _MASK64)) & _MASK64
    return h


def order_hash(indices):
    """sha256 of an order (indices into a file's examples), as hex"""
    return hashlib.sha256(np.asarray(list(indices), dtype=np.int64).tobytes()).hexdigest()


def fingerprint(command, args, *, hidden_dropout_prob, attention_probs_dropout_prob, train_batch_size=None, n_train=None,
                order=None, model=None, extra=None):
    """What must not change between the two halves of a run, as an ordered {field: value}.  n_train / order / model = None
    leave their fields out (the part of the fingerprint that is known before the data and the model are built).
    train_batch_size: the flag's value when args.train_batch_size has already been divided by --accumulate_gradients."""
    fp = {"command": command, "seed": int(args.seed),
          "train_batch_size": int(args.train_batch_size if train_batch_size is None else train_batch_size),
          "accumulate_gradients": int(args.accumulate_gradients),
          "gradient_accumulation_steps": int(args.gradient_accumulation_steps), "learning_rate": float(args.learning_rate),
          "weight_decay": float(args.weight_decay), "adam_epsilon": float(args.adam_epsilon),
          "max_grad_norm": float(args.max_grad_norm), "deterministic": bool(args.deterministic),
          "hidden_dropout_prob": float(hidden_dropout_prob), "attention_probs_dropout_prob": float(attention_probs_dropout_prob)}
    for k, v in (extra or {}).items():
        fp[k] = v
    if n_train is not None:
        fp["num_train_examples"] = int(n_train)
    if order is not None:
        fp["sampler_order_hash"] = order_hash(order)
    if model is not None:
        fp["model_keys"] = [[k, [int(s) for s in p.shape]] for k, p in model.named_parameters()]
    return fp


def check_fingerprint(saved, current, fields=None, what="--resume"):
    """SystemExit that names the first field (in the saved order) whose value differs; `fields` restricts the comparison,
    and a field that `current` does not carry yet is skipped."""
    for k, v in saved.items():
        if fields is not None and k not in fields:
            continue
        if k not in current:
            continue
        if k == "model_keys":
            have = [[a, list(b)] for a, b in current[k]]
            want = [[a, list(b)] for a, b in v]
            if have != want:
                first = next((f"{w} != {h}" for w, h in zip(want, have) if w != h), f"{len(want)} keys != {len(have)} keys")
                raise SystemExit(f"{what}: the state file was written by a different run: field 'model_keys' differs "
                                 f"(saved {first})")
        elif current[k] != v:
            raise SystemExit(f"{what}: the state file was written by a different run: field {k!r} is {current[k]!r} now, "
                             f"was {v!r} when the state was saved")
    missing = [k for k in current if k not in saved and (fields is None or k in fields)]
    if missing:
        raise SystemExit(f"{what}: the state file lacks the fingerprint field {missing[0]!r}")


def rng_states():
    """the states of `random`, `np.random` and torch's generators as plain containers and tensors"""
    version, internal, gauss = random.getstate()
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    out = {"python": [int(version), [int(x) for x in internal], gauss],
           "numpy": [str(kind), [int(x) for x in keys], int(pos), int(has_gauss), float(cached)],
           "torch": torch.get_rng_state()}
    if torch.cuda.is_available():
        out["torch_cuda"] = list(torch.cuda.get_rng_state_all())
    return out


def set_rng_states(states):
    version, internal, gauss = states["python"]
    random.setstate((version, tuple(internal), gauss))
    kind, keys, pos, has_gauss, cached = states["numpy"]
    np.random.set_state((kind, np.asarray(keys, dtype=np.uint32), pos, has_gauss, cached))
    torch.set_rng_state(states["torch"])
    if "torch_cuda" in states and torch.cuda.is_available() and len(states["torch_cuda"]) == torch.cuda.device_count():
        torch.cuda.set_rng_state_all(states["torch_cuda"])


def atomic_save(obj, path):
    """torch.save to `path`.tmp, fsync, rename over `path`, fsync of the directory: a write that is cut off leaves the
    previous file as it was."""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        torch.save(obj, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)
    try:
        fd = os.open(os.path.dirname(os.path.abspath(path)), os.O_RDONLY)
    except OSError:
        return
    try:
        os.fsync(fd)
    except OSError:
        pass
    finally:
        os.close(fd)


def resolve_state_path(path):
    """--resume PATH: a state file, or a run directory that holds trainer_state_last.pt"""
    if os.path.isdir(path):
        path = os.path.join(path, STATE_FILE)
    if not os.path.isfile(path):
        raise SystemExit(f"--resume: no state file at {path!r}")
    return path


def read_state(path):
    """the dict of a state file, checked for its format.  A `.tmp` beside it (a write that was cut off) is ignored."""
    try:
        obj = torch.load(path, map_location="cpu")
    except SystemExit:
        raise
    except Exception as e:
        raise SystemExit(f"--resume: {path!r} cannot be read as a state file ({type(e).__name__}: {e})")
    if not isinstance(obj, dict) or obj.get("format") != FORMAT:
        raise SystemExit(f"--resume: {path!r} is not a trainer state of format {FORMAT} (a model checkpoint goes to "
                         "--init_checkpoint)")
    for k in ("names", "shapes", "numel", "offsets", "flat", "digests", "trainer"):
        if k not in obj:
            raise SystemExit(f"--resume: {path!r} lacks {k!r}")
    return obj


def state_tensors(obj):
    """{name: fp32 tensor} views of a read state's flat buffer"""
    flat = obj["flat"]
    out = {}
    for name, shape, n, off in zip(obj["names"], obj["shapes"], obj["numel"], obj["offsets"]):
        out[name] = flat[off:off + 4 * n].view(torch.float32).reshape(shape)
    return out


def decode_device_state(words):
    """FusedAdamW.state_dict()['fused'] from the 16 fp32 words of the optimizer's device scalars"""
    raw = words.contiguous().view(torch.uint8).numpy()
    counters = raw[:24].view(np.int64)
    return {"step": int(counters[0]), "skipped_steps": int(counters[1]), "clean_steps": int(counters[2]),
            "loss_scale": float(raw[24:28].view(np.float32)[0])}


def trainer_state(*, fingerprint, global_step, batch_step, epoch, position, epoch_started, best, wait_step, stop_training,
                  dropout, losses, loss_steps, evals, param_groups, state_digests=(), fused=None, reader=None):
    """Everything beyond the tensors that determines the rest of the run.  `epoch` / `position`: the next micro-batch is
    number `position` of epoch `epoch`; epoch_started: that epoch's shuffle has been drawn.  fused = None: the writer
    decodes it from the snapshot's copy of the optimizer's device scalars."""
    return {"fingerprint": fingerprint, "global_step": int(global_step), "batch_step": int(batch_step), "epoch": int(epoch),
            "position": int(position), "epoch_started": bool(epoch_started), "best": float(best), "wait_step": int(wait_step),
            "stop_training": bool(stop_training), "dropout": [[int(s), int(c)] for s, c in dropout],
            "losses": [float(x) for x in losses], "loss_steps": [int(x) for x in loss_steps], "evals": list(evals),
            "param_groups": [dict(g) for g in param_groups], "state_digests": [dict(d) for d in state_digests],
            "fused": fused, "reader": reader}


# ---- the snapshotter -------------------------------------------------------------------------------------------------------

class StateSnapshotter:
    """tensors: fp32 CUDA tensors of one device, each contiguous (a view that starts anywhere inside a buffer is fine: a
    source needs 4-byte alignment only).  The tensors may change right after snapshot() returns: the kernel that copies
    them is already ordered before anything enqueued later on the same stream, and the file is written from the copy."""

    def __init__(self, tensors, names=None, device=None):
        self._lib = _lib.load()
        _lib.require_gpu()
        self.tensors = list(tensors)
        self.names = [f"t{i}" for i in range(len(self.tensors))] if names is None else list(names)
        if len(self.names) != len(self.tensors) or len(set(self.names)) != len(self.names):
            raise ValueError("StateSnapshotter: one distinct name per tensor")
        if device is None:
            device = self.tensors[0].device if self.tensors else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        for t in self.tensors:
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("StateSnapshotter takes contiguous fp32 CUDA tensors of one device")
        n = len(self.tensors)
        self.numel = np.array([t.numel() for t in self.tensors], dtype=np.int64)
        self.shapes = [[int(s) for s in t.shape] for t in self.tensors]
        offsets, self.nbytes = layout(self.numel)
        self.offsets = np.array(offsets, dtype=np.int64)
        lib = self._lib
        plan_bytes = int(lib.proqa_state_snapshot_plan_bytes(self.numel.ctypes.data, n))
        ws_bytes = int(lib.proqa_state_snapshot_workspace_bytes(self.numel.ctypes.data, n))
        if plan_bytes == 0 or ws_bytes == 0:
            _lib.check(-1)
        plan = np.zeros(plan_bytes, dtype=np.uint8)
        _lib.check(lib.proqa_state_snapshot_plan(self.numel.ctypes.data, self.offsets.ctypes.data, n, plan.ctypes.data, plan_bytes))
        with torch.cuda.device(self.device):
            self._ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=self.device)
            self._ws[:plan_bytes].copy_(torch.from_numpy(plan))
            self._digests = torch.zeros(max(n, 1), dtype=torch.int64, device=self.device)
            self._ptrs = torch.zeros(max(n, 1), dtype=torch.int64, device=self.device)
            self._side = torch.cuda.Stream(self.device)
        self._digests_host = torch.zeros(max(n, 1), dtype=torch.int64).pin_memory()
        self._flat = self._flat_host = None      # 4 bytes per element each: allocated by the first snapshot (prepare())
        self.refresh_pointers()
        self._thread = None
        self._error = None
        self._closed = False

    def refresh_pointers(self):
        """upload the tensors' addresses again (after a tensor of the list was replaced; `tensors[i] = new` first)"""
        if self.tensors:
            ptrs = np.array([t.data_ptr() for t in self.tensors], dtype=np.uint64).view(np.int64)
            with torch.cuda.device(self.device):
                self._ptrs.copy_(torch.from_numpy(ptrs))

    def prepare(self):
        """allocate the flat device buffer and its pinned host twin (the digest-only call needs neither).  The padding
        between tensors is zero and stays zero: the kernel never writes it."""
        if self._flat is None:
            with torch.cuda.device(self.device):
                self._flat = torch.zeros(max(self.nbytes, 1), dtype=torch.uint8, device=self.device)
            self._flat_host = torch.zeros(max(self.nbytes, 1), dtype=torch.uint8).pin_memory()

    def _launch(self, copy, digests):
        with torch.cuda.device(self.device):
            _lib.check(self._lib.proqa_state_snapshot(self._ptrs.data_ptr(), self.numel.ctypes.data, len(self.tensors),
                                                      self._flat.data_ptr() if copy else None,
                                                      self.offsets.ctypes.data if copy else None, digests.data_ptr(),
                                                      self._ws.data_ptr(), self._ws.numel(), _lib.current_stream_ptr()))

    def digest(self):
        """int64 device tensor [n_tensors]: the uint64 digests' bits, by the digest-only call on the current stream; no
        host wait.  (The call shares the snapshot's workspace: same stream as snapshot().)"""
        with torch.cuda.device(self.device):
            out = torch.empty(max(len(self.tensors), 1), dtype=torch.int64, device=self.device)
        if not self.tensors:
            return out[:0]
        self._launch(False, out)
        return out[:len(self.tensors)]

    def wait(self):
        """wait for the previous write; re-raises what it raised"""
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    def snapshot(self, path, meta=None, finish=None):
        """Enqueue the snapshot on the current stream and hand the write of `path` to the writer thread; returns without
        waiting for the device.  meta: the file's "trainer" entry.  finish(obj): called by the writer on the file's dict
        before it is saved (the tensors of state_tensors(obj) are final then)."""
        if self._closed:
            raise RuntimeError("StateSnapshotter is closed")
        self.wait()
        self.prepare()
        with torch.cuda.device(self.device):
            if self.tensors:
                self._launch(True, self._digests)
            main = torch.cuda.current_stream(self.device)
            taken = torch.cuda.Event()
            taken.record(main)
            self._side.wait_event(taken)
            with torch.cuda.stream(self._side):
                self._flat_host.copy_(self._flat, non_blocking=True)
                self._digests_host.copy_(self._digests, non_blocking=True)
                copied = torch.cuda.Event()
                copied.record(self._side)
            # the NEXT snapshot's kernel overwrites the flat buffer: it runs after wait(), which returns after `copied`
        self._thread = threading.Thread(target=self._write, args=(path, meta, finish, copied), daemon=True)
        self._thread.start()

    def _write(self, path, meta, finish, copied):
        try:
            while not copied.query():        # (a query is no synchronisation: the training thread's stream is not touched)
                time.sleep(0.0005)
            n = len(self.tensors)
            obj = {"format": FORMAT, "names": list(self.names), "shapes": [list(s) for s in self.shapes],
                   "numel": [int(x) for x in self.numel], "offsets": [int(x) for x in self.offsets],
                   "flat": self._flat_host[:self.nbytes], "digests": self._digests_host[:n], "trainer": meta}
            if finish is not None:
                finish(obj)
            atomic_save(obj, path)
        except BaseException as e:       # handed to the next wait()
            self._error = e

    def close(self):
        """wait for the last write; the buffers are released with the object"""
        self._closed = True
        self.wait()


# ---- model + optimizer -----------------------------------------------------------------------------------------------------

def _named_state(model, optimizer):
    names, tensors = [], []
    key_of = {}
    for k, p in model.named_parameters():
        names.append("model." + k)
        tensors.append(p.detach())
        key_of[id(p)] = k
    for kind in ("exp_avg", "exp_avg_sq"):
        for group in optimizer.param_groups:
            for p in group["params"]:
                if id(p) not in key_of:
                    raise ValueError("the optimizer holds a tensor that is not a parameter of the model")
                names.append(f"{kind}.{key_of[id(p)]}")
                tensors.append(optimizer.state[p][kind])
    if not getattr(optimizer, "_plain", True):
        names.append(DEVICE_STATE)
        tensors.append(optimizer._state_dev.view(torch.float32))
    return names, tensors


class TrainerCheckpoint:
    """The state of (model, FusedAdamW) as one snapshot: fp32 masters of every parameter, exp_avg and exp_avg_sq of the
    optimizer's, and its device scalars."""

    def __init__(self, model, optimizer):
        self.model, self.optimizer = model, optimizer
        names, tensors = _named_state(model, optimizer)
        self.snapshotter = StateSnapshotter(tensors, names)
        self._groups = {g: [i for i, n in enumerate(names) if n.startswith(prefix)]
                        for g, prefix in (("params", "model."), ("exp_avg", "exp_avg."), ("exp_avg_sq", "exp_avg_sq."))}

    def snapshot(self, path, trainer):
        """asynchronous (StateSnapshotter.snapshot); trainer: trainer_state(...)"""
        plain_fused = None
        if getattr(self.optimizer, "_plain", True):
            plain_fused = {"step": int(self.optimizer._plain_step), "loss_scale": 1.0, "clean_steps": 0, "skipped_steps": 0}

        def finish(obj):
            if obj["trainer"] is not None and obj["trainer"].get("fused") is None:
                obj["trainer"]["fused"] = plain_fused or decode_device_state(state_tensors(obj)[DEVICE_STATE])
        self.snapshotter.snapshot(path, trainer, finish)

    def digest(self):
        return self.snapshotter.digest()

    def group_digests(self, digests_host):
        """{params, exp_avg, exp_avg_sq}: one 64-bit number each from a host row of per-tensor digests, in key order"""
        return {g: combine_digests(int(digests_host[i]) for i in idx) for g, idx in self._groups.items()}

    def wait(self):
        self.snapshotter.wait()

    def close(self):
        self.snapshotter.close()

    def load(self, obj, what="--resume"):
        """Put a read_state() dict back: masters, both moments, the optimizer's scalars and its param-group
        hyper-parameters, the model's dropout state.  Then the digests are recomputed on the device and compared with the
        file's; the fp16 working copies are re-cast and an inference copy of the model is dropped.  Returns the file's
        "trainer" entry."""
        snap = self.snapshotter
        if list(obj["names"]) != snap.names:
            have, want = snap.names, list(obj["names"])
            first = next((f"{w!r} != {h!r}" for w, h in zip(want, have) if w != h), f"{len(want)} tensors != {len(have)}")
            raise SystemExit(f"{what}: the state file holds other tensors than this run's (saved {first})")
        for name, saved, have in zip(snap.names, obj["shapes"], snap.shapes):
            if list(saved) != list(have):
                raise SystemExit(f"{what}: tensor {name!r} has shape {list(have)} in this run, {list(saved)} in the state file")
        if obj["flat"].numel() < snap.nbytes or list(obj["offsets"]) != [int(x) for x in snap.offsets]:
            raise SystemExit(f"{what}: the state file's layout is not this run's")
        trainer = obj["trainer"]
        with torch.no_grad():
            for t, src in zip(snap.tensors, state_tensors(obj).values()):
                t.copy_(src)
        opt = self.optimizer
        if getattr(opt, "_plain", True):
            opt._plain_step = int(trainer["fused"]["step"])
        for group, saved in zip(opt.param_groups, trainer["param_groups"]):
            group["lr"], group["weight_decay"] = float(saved["lr"]), float(saved["weight_decay"])
        have = snap.digest().cpu().numpy()
        want = obj["digests"].numpy()
        for i, name in enumerate(snap.names):
            if int(have[i]) != int(want[i]):
                raise SystemExit(f"{what}: tensor {name!r} does not have the digest the state file records for it "
                                 f"({int(have[i]) & _MASK64:#018x} != {int(want[i]) & _MASK64:#018x}): the file is damaged")
        states = trainer["dropout"]
        self.model.set_dropout_state(states[0])
        if len(states) > 1 and hasattr(self.model, "retriever"):
            self.model.retriever.set_dropout_state(states[1])
        retriever = getattr(self.model, "retriever", self.model)
        retriever.refresh_half_weights()
        if hasattr(self.model, "_inference"):
            self.model._inference = None
        return trainer


class DigestLog:
    """--digest-every N: after every N-th update the digest-only call is enqueued; its results stay on the device until
    flush() reads them (with the losses: at an evaluation, a snapshot, the end).  entries: [{step, params, exp_avg,
    exp_avg_sq}], each value one 64-bit number combined from the per-tensor digests in key order."""

    def __init__(self, checkpoint, every, entries=()):
        self.checkpoint, self.every = checkpoint, int(every)
        self.entries = [dict(e) for e in entries]
        self._pending = []

    def after_update(self, global_step):
        if self.every > 0 and global_step % self.every == 0:
            self._pending.append((int(global_step), self.checkpoint.digest()))

    def flush(self, logger=None):
        if not self._pending:
            return
        rows = torch.stack([d for _, d in self._pending]).cpu().numpy()
        for (step, _), row in zip(self._pending, rows):
            entry = dict(step=step, **self.checkpoint.group_digests(row))
            self.entries.append(entry)
            if logger is not None:
                logger.info("state digest at step %d: params %016x exp_avg %016x exp_avg_sq %016x", step, entry["params"],
                            entry["exp_avg"], entry["exp_avg_sq"])
        self._pending = []


def dropout_states(model):
    """[(seed, call)] of the model and, for the reader, of its retriever"""
    out = [model.dropout_state()]
    if hasattr(model, "retriever"):
        out.append(model.retriever.dropout_state())
    return out


def save(path, model, optimizer, trainer):
    """one self-contained state file, written before this returns"""
    ck = TrainerCheckpoint(model, optimizer)
    try:
        ck.snapshot(path, trainer)
    finally:
        ck.close()


def load(path, model, optimizer, fingerprint=None):
    """restore a state file into (model, optimizer); fingerprint: this run's, compared with the file's first.  Returns the
    "trainer" entry."""
    obj = read_state(resolve_state_path(path))
    if fingerprint is not None:
        check_fingerprint(obj["trainer"]["fingerprint"], fingerprint)
    ck = TrainerCheckpoint(model, optimizer)
    try:
        return ck.load(obj)
    finally:
        ck.close()
