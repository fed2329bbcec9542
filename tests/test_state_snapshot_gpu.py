"""proqa_state_snapshot on the MI355X against tests/state_digest_oracle.py, exactly: the copied bytes are the sources'
bits and every digest is the oracle's number.  The shapes sit where the kernel changes its path: CHUNK (elements of one
tensor per workgroup, PROQA_STATE_CHUNK = 16384) minus and plus one and two chunks plus three, sizes around one 16-byte
vector, sources that start 1, 2 and 3 elements into a buffer (only 4-byte aligned: scalar head, 16-byte body, scalar
tail, 4-byte stores), 0, 1 and 500 tensors (500 is more than the four tensors one finishing workgroup serves, and more
than one wave of them)."""
import os

import numpy as np
import pytest
import torch

import state_digest_oracle as oracle

pytestmark = pytest.mark.gpu

CHUNK = oracle.CHUNK
FILL = 0xA5


def _bits(rng, n):
    """random 32-bit patterns (NaNs with payloads, infinities and denormals among them) with the special values planted"""
    b = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x80000000, 0x00000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0x807FFFFF, 0x7F800000],
                       dtype=np.uint32)          # -0.0, 0.0, quiet and signalling NaNs with payloads, denormals, inf
    k = min(n, len(special))
    b[:k] = special[:k]
    return b


def _device_tensors(dev, bit_arrays, shifts=None):
    """fp32 CUDA tensors holding exactly these bits; shifts[i] > 0: tensor i is a view that starts `shift` elements into
    its own 16-byte aligned buffer"""
    out = []
    for i, b in enumerate(bit_arrays):
        shift = 0 if shifts is None else shifts[i]
        buf = torch.zeros(shift + len(b) + 4, dtype=torch.int32, device=dev)
        assert buf.data_ptr() % 16 == 0
        view = buf[shift:shift + len(b)]
        view.copy_(torch.from_numpy(b.view(np.int32)))
        t = view.view(torch.float32)
        assert t.is_contiguous() and (len(b) == 0 or t.data_ptr() % 16 == (4 * shift) % 16)
        out.append(t)
    return out


def _run(lib, dev, tensors, copy=True):
    """one raw call -> (digests as Python ints, the flat buffer's bytes or None, offsets, total)"""
    from proqa_amd import _lib
    n = len(tensors)
    numel = np.array([t.numel() for t in tensors], dtype=np.int64)
    offsets, total = oracle.layout(numel)
    off = np.array(offsets, dtype=np.int64)
    plan_bytes = lib.proqa_state_snapshot_plan_bytes(numel.ctypes.data, n)
    ws_bytes = lib.proqa_state_snapshot_workspace_bytes(numel.ctypes.data, n)
    assert plan_bytes > 0 and ws_bytes > plan_bytes
    image = np.zeros(plan_bytes, dtype=np.uint8)
    _lib.check(lib.proqa_state_snapshot_plan(numel.ctypes.data, off.ctypes.data, n, image.ctypes.data, plan_bytes))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    ws[:plan_bytes].copy_(torch.from_numpy(image))
    ptrs = torch.from_numpy(np.array([t.data_ptr() for t in tensors] + [0], dtype=np.uint64).view(np.int64)).to(dev)
    digests = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    flat = torch.full((total + 256,), FILL, dtype=torch.uint8, device=dev) if copy else None
    _lib.check(lib.proqa_state_snapshot(ptrs.data_ptr(), numel.ctypes.data, n, flat.data_ptr() if copy else None,
                                        off.ctypes.data if copy else None, digests.data_ptr(), ws.data_ptr(), ws_bytes,
                                        _lib.current_stream_ptr()))
    d = digests.cpu().numpy()
    assert d[n] == -1                                                  # nothing behind the last digest was written
    return [int(x) & ((1 << 64) - 1) for x in d[:n]], (flat.cpu().numpy() if copy else None), offsets, total


def _check_copy(flat, offsets, total, bit_arrays):
    """every tensor's bytes are its bits; every byte between tensors and behind the last keeps the prefill"""
    touched = np.zeros(len(flat), dtype=bool)
    for off, b in zip(offsets, bit_arrays):
        got = flat[off:off + 4 * len(b)].view(np.uint32)
        assert np.array_equal(got, b)
        touched[off:off + 4 * len(b)] = True
    assert (flat[~touched] == FILL).all() and len(flat) == total + 256


SETS = {
    "around_a_vector": ([0, 1, 3, 4, 5], None),
    "around_a_chunk": ([CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3], None),
    "shifted_sources": ([1000, CHUNK + 5, 7, 2, 2 * CHUNK + 3, 1], [1, 2, 3, 3, 1, 2]),
    "one_tensor": ([777], None),
}


@pytest.fixture(scope="module")
def cases(gpu_device):
    """name -> (bit arrays, device tensors, oracle digests), computed once"""
    rng = np.random.default_rng(7)
    out = {}
    sets = dict(SETS)
    sizes500 = [int(x) for x in rng.integers(0, 300, size=500)]
    sizes500[17], sizes500[250], sizes500[499] = CHUNK + 1, 0, 4 * 256 + 2
    sets["five_hundred"] = (sizes500, [int(x) for x in rng.integers(0, 4, size=500)])
    for name, (sizes, shifts) in sets.items():
        arrays = [_bits(rng, n) for n in sizes]
        out[name] = (arrays, _device_tensors(gpu_device, arrays, shifts), [oracle.digest(b) for b in arrays])
    return out


@pytest.mark.parametrize("name", list(SETS) + ["five_hundred"])
def test_copy_and_digests_are_the_oracles(gpu_device, cases, name):
    from proqa_amd import _lib
    arrays, tensors, want = cases[name]
    digests, flat, offsets, total = _run(_lib.load(), gpu_device, tensors)
    assert digests == want
    _check_copy(flat, offsets, total, arrays)
    # digest-only mode gives the same digests, and a second run the same bits
    only, none, _, _ = _run(_lib.load(), gpu_device, tensors, copy=False)
    assert only == want and none is None
    again, flat2, _, _ = _run(_lib.load(), gpu_device, tensors)
    assert again == digests and np.array_equal(flat2, flat)
    # the sources are untouched
    for t, b in zip(tensors, arrays):
        assert np.array_equal(t.view(torch.int32).cpu().numpy().view(np.uint32), b)


def test_no_tensors_and_empty_tensors(gpu_device):
    from proqa_amd import _lib
    from proqa_amd.checkpoint import StateSnapshotter
    lib = _lib.load()
    assert lib.proqa_state_snapshot(None, None, 0, None, None, None, None, 0, _lib.current_stream_ptr()) == 0
    empty = [torch.empty(0, dtype=torch.float32, device=gpu_device) for _ in range(3)]
    digests, flat, offsets, total = _run(lib, gpu_device, empty)
    assert digests == [0, 0, 0] and total == 0 and (flat == FILL).all()
    snap = StateSnapshotter([], device=gpu_device)
    assert snap.digest().numel() == 0
    snap.close()


def test_one_bit_and_a_swap_change_the_device_digest(gpu_device, cases):
    from proqa_amd import _lib
    arrays, _, want = cases["around_a_chunk"]
    b = arrays[3].copy()
    b[2 * CHUNK + 1] ^= np.uint32(1)
    c = arrays[3].copy()
    c[5], c[CHUNK + 9] = arrays[3][CHUNK + 9], arrays[3][5]
    assert c[5] != c[CHUNK + 9]
    digests, _, _, _ = _run(_lib.load(), gpu_device, _device_tensors(gpu_device, [b, c]), copy=False)
    assert digests == [oracle.digest(b), oracle.digest(c)] and want[3] not in digests


# ---- StateSnapshotter --------------------------------------------------------------------------------------------------------

def _file_bits(obj, name):
    from proqa_amd.checkpoint import state_tensors
    return state_tensors(obj)[name].contiguous().view(torch.int32).numpy().view(np.uint32).reshape(-1)


def test_snapshot_does_not_wait_and_isolates_the_file(gpu_device, cases, tmp_path):
    """snapshot() under the sync debug mode of tests/test_optim_gpu.py; then every source changes on the same stream
    before the file is written: the file holds the values from before"""
    from proqa_amd import checkpoint
    arrays, _, want = cases["shifted_sources"]
    _, shifts = SETS["shifted_sources"]
    tensors = _device_tensors(gpu_device, arrays, shifts)
    names = [f"model.t{i}" for i in range(len(tensors))]
    snap = checkpoint.StateSnapshotter(tensors, names)
    snap.prepare()
    snap._flat.fill_(FILL)                      # the padding between tensors must survive the kernel
    path = str(tmp_path / "state.pt")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        snap.snapshot(path, {"global_step": 5})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for t in tensors:
        t.add_(1)
    snap.close()
    obj = checkpoint.read_state(path)
    assert obj["names"] == names and obj["trainer"] == {"global_step": 5} and not os.path.exists(path + ".tmp")
    assert [int(d) & ((1 << 64) - 1) for d in obj["digests"].tolist()] == want
    flat = obj["flat"].numpy()
    touched = np.zeros(len(flat), dtype=bool)
    for name, b, off in zip(names, arrays, obj["offsets"]):
        assert np.array_equal(_file_bits(obj, name), b)
        touched[off:off + 4 * len(b)] = True
    assert (flat[~touched] == FILL).all()
    # the sources did change
    moved = tensors[0].view(torch.int32).cpu().numpy().view(np.uint32)
    assert not np.array_equal(moved, arrays[0])
    with pytest.raises(RuntimeError, match="closed"):
        snap.snapshot(path, None)


def test_second_snapshot_replaces_the_first_and_digest_call_matches(gpu_device, tmp_path):
    from proqa_amd import checkpoint
    rng = np.random.default_rng(3)
    arrays = [_bits(rng, n) for n in (CHUNK + 1, 33)]
    tensors = _device_tensors(gpu_device, arrays)
    snap = checkpoint.StateSnapshotter(tensors, ["model.a", "model.b"])
    path = str(tmp_path / checkpoint.STATE_FILE)
    snap.snapshot(path, {"n": 1})
    tensors[1].view(torch.int32).fill_(0x7FC00001)       # NaNs with a payload: a float compare would lose them
    snap.snapshot(path, {"n": 2})                        # waits for the first write
    d = snap.digest()
    snap.close()
    obj = checkpoint.read_state(checkpoint.resolve_state_path(str(tmp_path)))
    assert obj["trainer"] == {"n": 2}
    assert np.array_equal(_file_bits(obj, "model.a"), arrays[0])
    assert (_file_bits(obj, "model.b") == 0x7FC00001).all()
    assert d.tolist() == obj["digests"].tolist()
    assert int(d[1]) & ((1 << 64) - 1) == oracle.digest(np.full(33, 0x7FC00001, dtype=np.uint32))


def test_refusals(gpu_device):
    from proqa_amd import checkpoint
    with pytest.raises(ValueError, match="contiguous fp32 CUDA"):
        checkpoint.StateSnapshotter([torch.zeros(4, 4, device=gpu_device)[:, 1]])
    with pytest.raises(ValueError, match="contiguous fp32 CUDA"):
        checkpoint.StateSnapshotter([torch.zeros(4, dtype=torch.float16, device=gpu_device)])
    with pytest.raises(ValueError, match="distinct name"):
        checkpoint.StateSnapshotter([torch.zeros(4, device=gpu_device)] * 2, ["a", "a"])
