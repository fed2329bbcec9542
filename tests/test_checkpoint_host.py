"""What of the checkpoint / resume subsystem can be checked without a GPU: the digest's restatement and its two promised
separations, the additive C ABI (version 7, pure host size and plan functions, the refusal of tensors beyond 2^31
elements), the fingerprint check, the flags of both commands, the atomic write, and the sampler's permutation."""
import argparse
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import state_digest_oracle as oracle
from proqa_amd import _lib, checkpoint, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the digest ------------------------------------------------------------------------------------------------------------

def test_oracle_constants_are_the_headers():
    header = open(os.path.join(ROOT, "include", "proqa_hip.h")).read()
    assert int(re.search(r"#define PROQA_STATE_MIX_XOR (0x[0-9A-Fa-f]+)u", header).group(1), 16) == oracle.MIX_XOR == _lib.STATE_MIX_XOR
    assert int(re.search(r"#define PROQA_STATE_CHUNK (\d+)", header).group(1)) == oracle.CHUNK == _lib.STATE_CHUNK
    assert int(re.search(r"#define PROQA_STATE_DST_ALIGN (\d+)", header).group(1)) == oracle.DST_ALIGN == _lib.STATE_DST_ALIGN


def test_digest_by_hand_and_empty():
    assert oracle.digest(np.zeros(0, dtype=np.float32)) == 0
    b = np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32)
    want = sum(((int(x) ^ 0x9E3779B9) * (2 * i + 1)) for i, x in enumerate(b)) % (1 << 64)
    assert oracle.digest(b) == want
    # the sum wraps mod 2^64: 2^31 - 1 is the largest index, its weight 2^32 - 1
    assert int(oracle.mix(np.uint32(0x61C88646), np.uint64((1 << 31) - 1))) == ((0x61C88646 ^ 0x9E3779B9) * ((1 << 32) - 1)) % (1 << 64)
    # a zero-filled tensor's digest depends on its length
    assert oracle.digest(np.zeros(5, np.float32)) != oracle.digest(np.zeros(6, np.float32)) != 0


def test_one_bit_and_swaps_change_the_digest():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(4099).astype(np.float32)
    base = oracle.digest(x)
    bits = oracle.bits_of(x)
    for i in (0, 1, 2048, 4098):
        for bit in (0, 13, 31):
            y = bits.copy()
            y[i] ^= np.uint32(1 << bit)
            assert oracle.digest(y) != base, (i, bit)
    for i, j in ((0, 1), (0, 4098), (17, 18), (1000, 3000)):
        assert bits[i] != bits[j]
        y = bits.copy()
        y[i], y[j] = bits[j], bits[i]
        assert oracle.digest(y) != base, (i, j)
    # position sensitive even for values that differ in the top bit only (0.0 and -0.0)
    z = np.zeros(8, dtype=np.float32)
    z[3] = -0.0
    w = np.zeros(8, dtype=np.float32)
    w[4] = -0.0
    assert oracle.digest(z) != oracle.digest(w) != oracle.digest(np.zeros(8, np.float32))


def test_combine_digests_is_order_sensitive():
    assert checkpoint.combine_digests([]) == 0
    assert checkpoint.combine_digests([1, 2]) != checkpoint.combine_digests([2, 1])
    assert checkpoint.combine_digests([-1]) == (1 << 64) - 1          # an int64 bit pattern is read as uint64
    assert 0 <= checkpoint.combine_digests([(1 << 64) - 1] * 50) < 1 << 64


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------

def _sizes(values):
    return np.array(values, dtype=np.int64)


def test_abi_version_and_host_size_functions():
    lib = _lib.load()
    assert lib.proqa_abi_version() == 7
    C = oracle.CHUNK
    numel = _sizes([0, 1, C - 1, C, C + 1, 2 * C + 3])
    n_chunks = 0 + 1 + 1 + 1 + 2 + 3
    plan = lib.proqa_state_snapshot_plan_bytes(numel.ctypes.data, len(numel))
    assert plan == -(-(32 * len(numel) + 8 * n_chunks) // 16) * 16
    assert lib.proqa_state_snapshot_workspace_bytes(numel.ctypes.data, len(numel)) == plan + 8 * n_chunks
    # no tensors, and tensors without elements: valid, a minimal workspace
    assert lib.proqa_state_snapshot_workspace_bytes(None, 0) == 32
    empty = _sizes([0, 0])
    assert lib.proqa_state_snapshot_workspace_bytes(empty.ctypes.data, 2) == 64 + 16
    # 2^31 elements are the limit; one more is refused, not mis-indexed
    assert lib.proqa_state_snapshot_workspace_bytes(_sizes([1 << 31]).ctypes.data, 1) > 0
    big = _sizes([5, (1 << 31) + 1])
    assert lib.proqa_state_snapshot_workspace_bytes(big.ctypes.data, 2) == 0
    assert b"more than 2^31" in lib.proqa_last_error()
    assert lib.proqa_state_snapshot_plan_bytes(_sizes([-1]).ctypes.data, 1) == 0
    # the launch function validates on the host before it touches a device: same refusal, PROQA_EINVAL
    status = lib.proqa_state_snapshot(None, big.ctypes.data, 2, None, None, None, None, 0, None)
    assert status < 0 and b"tensor 1" in lib.proqa_last_error()
    assert lib.proqa_state_snapshot(None, None, 0, None, None, None, None, 0, None) == 0       # nothing to do


def test_plan_image():
    lib = _lib.load()
    C = oracle.CHUNK
    numel = _sizes([3, 0, 2 * C + 3, C])
    offsets, total = oracle.layout(numel)
    assert offsets == [0, 256, 256, 256 + (-(-(2 * C + 3) * 4 // 256)) * 256]
    off = _sizes(offsets)
    nbytes = lib.proqa_state_snapshot_plan_bytes(numel.ctypes.data, 4)
    image = np.zeros(nbytes, dtype=np.uint8)
    assert lib.proqa_state_snapshot_plan(numel.ctypes.data, off.ctypes.data, 4, image.ctypes.data, nbytes) == 0
    tensors = image[:4 * 32].view(np.int64).reshape(4, 4)
    assert tensors.tolist() == [[3, offsets[0], 0, 1], [0, offsets[1], 1, 0], [2 * C + 3, offsets[2], 1, 3], [C, offsets[3], 4, 1]]
    chunks = image[4 * 32:4 * 32 + 5 * 8].view(np.int32).reshape(5, 2)
    assert chunks.tolist() == [[0, 0], [2, 0], [2, 1], [2, 2], [3, 0]]
    # a destination that is not on a 256-byte boundary, and an image that is too small
    bad = _sizes([0, 256, 300, 1024])
    assert lib.proqa_state_snapshot_plan(numel.ctypes.data, bad.ctypes.data, 4, image.ctypes.data, nbytes) < 0
    assert b"tensor 2" in lib.proqa_last_error()
    assert lib.proqa_state_snapshot_plan(numel.ctypes.data, off.ctypes.data, 4, image.ctypes.data, nbytes - 16) < 0
    assert checkpoint.layout(numel) == (offsets, total)


def test_signatures_are_bound():
    for name in ("proqa_state_snapshot", "proqa_state_snapshot_plan", "proqa_state_snapshot_plan_bytes",
                 "proqa_state_snapshot_workspace_bytes"):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["proqa_state_snapshot"][1][-1] is ctypes.c_void_p and len(_lib.SIGNATURES["proqa_state_snapshot"][1]) == 9


# ---- fingerprint -------------------------------------------------------------------------------------------------------------

class _Model:
    def __init__(self, shapes):
        self.shapes = shapes

    def named_parameters(self):
        return [(k, torch.empty(s)) for k, s in self.shapes.items()]


def _fingerprint(**changes):
    args = argparse.Namespace(seed=3, train_batch_size=8, accumulate_gradients=2, gradient_accumulation_steps=2, learning_rate=1e-5,
                              weight_decay=0.01, adam_epsilon=1e-8, max_grad_norm=2.0, deterministic=True)
    kw = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, n_train=32, order=list(range(32)),
              model=_Model({"a.weight": (4, 3), "a.bias": (4,)}), extra={"qa_drop": 0.0})
    for k, v in changes.items():
        if hasattr(args, k):
            setattr(args, k, v)
        else:
            kw[k] = v
    return checkpoint.fingerprint("pretrain_retriever.py", args, **kw)


CHANGES = {"seed": 4, "train_batch_size": 16, "accumulate_gradients": 1, "gradient_accumulation_steps": 1, "learning_rate": 2e-5,
           "weight_decay": 0.0, "adam_epsilon": 1e-6, "max_grad_norm": 5.0, "deterministic": False, "hidden_dropout_prob": 0.0,
           "attention_probs_dropout_prob": 0.2, "n_train": 31, "order": list(range(31, -1, -1)),
           "model": _Model({"a.weight": (4, 3), "a.bias": (5,)}), "extra": {"qa_drop": 0.1}}
FIELD_OF = {"n_train": "num_train_examples", "order": "sampler_order_hash", "model": "model_keys", "extra": "qa_drop"}


def test_fingerprint_fields():
    fp = _fingerprint()
    assert set(fp) == {"command", "seed", "train_batch_size", "accumulate_gradients", "gradient_accumulation_steps",
                       "learning_rate", "weight_decay", "adam_epsilon", "max_grad_norm", "deterministic", "hidden_dropout_prob",
                       "attention_probs_dropout_prob", "qa_drop", "num_train_examples", "sampler_order_hash", "model_keys"}
    assert fp["model_keys"] == [["a.weight", [4, 3]], ["a.bias", [4]]]
    checkpoint.check_fingerprint(fp, _fingerprint())          # equal: no refusal
    assert set(CHANGES) | {"command"} >= {k for k in fp if k not in FIELD_OF.values()}


@pytest.mark.parametrize("changed", sorted(CHANGES))
def test_fingerprint_mismatch_names_the_field(changed):
    field = FIELD_OF.get(changed, changed)
    with pytest.raises(SystemExit, match=f"'{field}'"):
        checkpoint.check_fingerprint(_fingerprint(), _fingerprint(**{changed: CHANGES[changed]}))


def test_fingerprint_of_the_flags_alone_is_checked_first():
    early = checkpoint.fingerprint("train_reader.py", argparse.Namespace(
        seed=9, train_batch_size=8, accumulate_gradients=2, gradient_accumulation_steps=2, learning_rate=1e-5, weight_decay=0.01,
        adam_epsilon=1e-8, max_grad_norm=2.0, deterministic=True), hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    assert "model_keys" not in early and "num_train_examples" not in early
    with pytest.raises(SystemExit, match="'command'"):
        checkpoint.check_fingerprint(_fingerprint(), early, fields=tuple(early))
    early["command"] = "pretrain_retriever.py"
    with pytest.raises(SystemExit, match="'seed' is 9 now, was 3"):
        checkpoint.check_fingerprint(_fingerprint(), early, fields=tuple(early))


# ---- flags -------------------------------------------------------------------------------------------------------------------

def test_flags_of_both_commands():
    from proqa_amd import pretrain_retriever, train_reader
    for get_args in (config.get_args, train_reader.get_args):
        a = get_args([])
        assert (a.save_state, a.stop_after_updates, a.resume, a.digest_every) == (False, 0, "", 0)
        a = get_args(["--save-state", "--stop-after-updates", "7", "--resume", "run/dir", "--digest-every", "2"])
        assert (a.save_state, a.stop_after_updates, a.resume, a.digest_every) == (True, 7, "run/dir", 2)
    base = ["--train_file", "t.txt", "--predict_file", "d.txt"]
    a = pretrain_retriever.check_args(config.get_args(base + ["--stop-after-updates", "3"]))
    assert a.save_state is True                                   # implied
    assert pretrain_retriever.check_args(config.get_args(base)).save_state is False
    a = train_reader.check_args(train_reader.get_args(["--matched-para-path", "m.txt", "--stop-after-updates", "3"]))
    assert a.save_state is True
    with pytest.raises(SystemExit, match="--resume together with --init_checkpoint"):
        pretrain_retriever.check_args(config.get_args(base + ["--resume", "x.pt", "--init_checkpoint", "y.pt"]))
    with pytest.raises(SystemExit, match="--resume together with --init_checkpoint"):
        train_reader.check_args(train_reader.get_args(["--matched-para-path", "m.txt", "--resume", "x.pt", "--init_checkpoint", "y.pt"]))
    with pytest.raises(SystemExit, match="negative"):
        pretrain_retriever.check_args(config.get_args(base + ["--digest-every", "-1"]))


# ---- the file ------------------------------------------------------------------------------------------------------------------

def _state(value):
    flat = torch.zeros(256 + 12, dtype=torch.uint8)
    flat[:8] = torch.tensor([value, 2.0], dtype=torch.float32).view(torch.uint8)
    flat[256:268] = torch.tensor([3.0, 4.0, 5.0], dtype=torch.float32).view(torch.uint8)
    return {"format": checkpoint.FORMAT, "names": ["model.a", "model.b"], "shapes": [[2], [3, 1]], "numel": [2, 3],
            "offsets": [0, 256], "flat": flat, "digests": torch.tensor([1, -2], dtype=torch.int64),
            "trainer": {"global_step": int(value), "rng": checkpoint.rng_states()}}


def test_atomic_write_keeps_the_old_file(tmp_path, monkeypatch):
    path = str(tmp_path / checkpoint.STATE_FILE)
    checkpoint.atomic_save(_state(1.0), path)
    assert not os.path.exists(path + ".tmp")
    good = open(path, "rb").read()
    # the process died between the write of .tmp and the rename: a truncated .tmp lies beside the good file
    with open(path + ".tmp", "wb") as f:
        f.write(good[:len(good) // 2])
    obj = checkpoint.read_state(checkpoint.resolve_state_path(str(tmp_path)))       # the run directory names the file
    assert obj["trainer"]["global_step"] == 1
    t = checkpoint.state_tensors(obj)
    assert t["model.a"].tolist() == [1.0, 2.0] and t["model.b"].shape == (3, 1) and t["model.b"].flatten().tolist() == [3.0, 4.0, 5.0]
    # ... or in the rename itself: the old file is untouched, the next write replaces the stale .tmp and the file
    real = os.replace
    monkeypatch.setattr(os, "replace", lambda a, b: (_ for _ in ()).throw(OSError("killed")))
    with pytest.raises(OSError, match="killed"):
        checkpoint.atomic_save(_state(2.0), path)
    assert open(path, "rb").read() == good
    monkeypatch.setattr(os, "replace", real)
    checkpoint.atomic_save(_state(3.0), path)
    assert checkpoint.read_state(path)["trainer"]["global_step"] == 3 and not os.path.exists(path + ".tmp")
    # the truncated file itself is refused with a message, not a traceback
    with open(path, "wb") as f:
        f.write(good[:len(good) // 2])
    with pytest.raises(SystemExit, match="cannot be read as a state file"):
        checkpoint.read_state(path)


def test_read_state_refusals(tmp_path):
    with pytest.raises(SystemExit, match="no state file"):
        checkpoint.resolve_state_path(str(tmp_path))
    model_ckpt = str(tmp_path / "checkpoint_last.pt")
    torch.save({"proj_q.weight": torch.zeros(2, 2)}, model_ckpt)
    with pytest.raises(SystemExit, match="--init_checkpoint"):
        checkpoint.read_state(model_ckpt)


def test_rng_states_round_trip():
    random.seed(5)
    np.random.seed(6)
    torch.manual_seed(7)
    random.random(), np.random.rand(3), torch.rand(2)
    saved = checkpoint.rng_states()
    want = (random.random(), np.random.rand(2).tolist(), torch.rand(2).tolist(), random.sample(range(100), 5))
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    checkpoint.set_rng_states(saved)
    assert (random.random(), np.random.rand(2).tolist(), torch.rand(2).tolist(), random.sample(range(100), 5)) == want


def test_decode_device_state():
    raw = np.zeros(64, dtype=np.uint8)
    raw[:24].view(np.int64)[:] = [12, 3, 7]
    raw[24:28].view(np.float32)[0] = 32768.0
    words = torch.from_numpy(raw.view(np.float32).copy())
    assert checkpoint.decode_device_state(words) == {"step": 12, "skipped_steps": 3, "clean_steps": 7, "loss_scale": 32768.0}


# ---- the sampler's permutation -------------------------------------------------------------------------------------------------

def test_sampler_shuffle_tracks_its_permutation():
    """OnlineSampler.shuffle() arranges qa_data as random.shuffle(qa_data) did, draws the same numbers, and knows the
    permutation; a saved permutation and `random` state continue as the uninterrupted sampler does."""
    from proqa_amd.online_sampler import OnlineSampler
    data = [{"question": f"q{i}"} for i in range(23)]

    def sampler():
        s = OnlineSampler.__new__(OnlineSampler)
        s.qa_data, s._file_data, s._order = list(data), list(data), list(range(len(data)))
        return s
    a = sampler()
    random.seed(4)
    a.shuffle()
    a.shuffle()
    after = random.random()
    plain = list(data)
    random.seed(4)
    random.shuffle(plain)
    random.shuffle(plain)
    assert a.qa_data == plain and random.random() == after
    assert [data[i] for i in a.permutation()] == plain
    # resume after the first shuffle
    b = sampler()
    random.seed(4)
    b.shuffle()
    saved, state = b.permutation(), random.getstate()
    c = sampler()
    random.seed(99)
    c.set_permutation(saved)
    random.setstate(state)
    c.shuffle()
    assert c.qa_data == plain
    with pytest.raises(ValueError, match="not a permutation"):
        c.set_permutation([0] * 23)
