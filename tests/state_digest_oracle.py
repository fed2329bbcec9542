"""NumPy restatement of proqa_state_snapshot's digest and layout (include/proqa_hip.h):

    digest(t) = sum over i of mix(bits_i, i) mod 2^64,   mix(bits, i) = ((bits ^ 0x9E3779B9) * (2 i + 1)) mod 2^64

over the 32-bit patterns of the tensor's fp32 words; an empty tensor has digest 0.  uint64 array arithmetic wraps mod 2^64.
"""
import numpy as np

MIX_XOR = 0x9E3779B9
CHUNK = 16384        # PROQA_STATE_CHUNK: elements of one tensor per workgroup
DST_ALIGN = 256      # PROQA_STATE_DST_ALIGN


def bits_of(array):
    """the uint32 patterns of an fp32 (or already uint32) array, flattened"""
    a = np.ascontiguousarray(array)
    if a.dtype == np.float32:
        a = a.view(np.uint32)
    assert a.dtype == np.uint32
    return a.reshape(-1)


def mix(bits, index):
    bits = np.asarray(bits, dtype=np.uint64)
    index = np.asarray(index, dtype=np.uint64)
    return (bits ^ np.uint64(MIX_XOR)) * (np.uint64(2) * index + np.uint64(1))


def digest(array):
    """the digest as a Python int in [0, 2^64)"""
    b = bits_of(array)
    if b.size == 0:
        return 0
    return int(mix(b, np.arange(b.size, dtype=np.uint64)).sum(dtype=np.uint64))


def layout(numels):
    """(byte offsets, total bytes) of tensors laid out on DST_ALIGN-byte boundaries"""
    offsets, at = [], 0
    for n in numels:
        offsets.append(at)
        at += -(-(int(n) * 4) // DST_ALIGN) * DST_ALIGN
    return offsets, at
