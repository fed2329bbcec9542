"""Folded passage texts in HBM and the answer pre-filter that runs on them (csrc/text_match_kernels.hip).

`eval_retrieval.para_has_answer` tokenises a paragraph only if `_may_match` finds every token of some alias in the folded
paragraph as a substring.  TextStore keeps the folded texts of the whole corpus on the device, addressed by index row, so that
this test runs where the search leaves its candidate rows: one bit per (question, slot) comes back instead of the lists.

    blob, spans, seconds = fold_sidecar("idx_id.txt", workers=16)      # host only: fork its pool BEFORE any HIP call
    store = TextStore(blob, spans)                                      # upload
    needles = NeedleTable([needles_of(answer) for answer in answers])  # folded tokens per alias, per question
    mask, count = store.prefilter(I_dev, needles)                       # int32 [nq, ceil(k/32)] (the bits), int32 [nq]

Folding is `_fold(normalize(text))` in UTF-8: NFD, str.lower(), final sigma -> sigma.  UTF-8 is self-synchronising, so a byte
substring of the folded text is a character substring and the device compares bytes.
"""
import ctypes
import time

import numpy as np

from . import _lib
from .eval_retrieval import _fold
from .utils import normalize

MAX_TOKEN_BYTES = 255
MAX_TOKENS = 128          # distinct tokens per question
MAX_ALIASES = 64
MAX_NEEDLE_BYTES = 4096   # per question
MAX_K = 16384


def fold(text):
    """The bytes the device searches: eval_retrieval._fold(normalize(text)) in UTF-8."""
    return _fold(normalize(text)).encode("utf-8")


def fold_needles(needles):
    """[[token, ...] per alias] (the words of each alias, as para_has_answer forms them) -> the same with folded bytes"""
    return [[_fold(tok).encode("utf-8") for tok in alias] for alias in needles]


def within_limits(folded_needles):
    """True if a question's folded needles fit the kernel's limits; the others take the host route."""
    if len(folded_needles) > MAX_ALIASES:
        return False
    distinct = {tok for alias in folded_needles for tok in alias}
    return (len(distinct) <= MAX_TOKENS and sum(len(t) for t in distinct) <= MAX_NEEDLE_BYTES
            and all(1 <= len(t) <= MAX_TOKEN_BYTES for t in distinct))


def _fold_span_chunk(args):
    """worker: the folded texts of the spans [lo, hi) of a sidecar's blob, joined, and their lengths"""
    txt_path, spans = args
    import os
    blob = np.memmap(txt_path, dtype=np.uint8, mode="r") if os.path.getsize(txt_path) > 0 else np.zeros(0, np.uint8)
    out = [fold(bytes(blob[int(lo):int(hi)]).decode("utf-8")) for lo, hi in spans]
    return b"".join(out), np.asarray([len(b) for b in out], dtype=np.int64)


def fold_sidecar(txt_path, workers=0, pool=None, chunk=4096):
    """Fold every distinct text of a text sidecar (gen_index_id_map.write_text_sidecar).  Returns (blob bytes-like, spans
    int64 [rows, 2], seconds).  `pool`: a multiprocessing pool to run on; otherwise `workers` > 1 forks one here -- do that
    before the process touches the GPU.  Rows that share a text in the sidecar share its folded copy."""
    t0 = time.perf_counter()
    raw = np.asarray(np.load(txt_path[:-4] + ".txtoff.npy")).reshape(-1, 2).astype(np.int64)
    distinct, inverse = np.unique(raw, axis=0, return_inverse=True) if len(raw) else (raw, np.zeros(0, np.int64))
    inverse = np.asarray(inverse).reshape(-1)
    jobs = [(txt_path, distinct[i:i + chunk]) for i in range(0, len(distinct), chunk)]
    own = None
    if pool is None and workers > 1 and len(jobs) > 1:
        from multiprocessing import Pool
        pool = own = Pool(processes=workers)
    try:
        parts = pool.map(_fold_span_chunk, jobs) if pool is not None else [_fold_span_chunk(j) for j in jobs]
    finally:
        if own is not None:
            own.close()
            own.join()
    lens = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.int64)
    ends = np.cumsum(lens)
    folded = np.stack([ends - lens, ends], axis=1) if len(lens) else np.zeros((0, 2), np.int64)
    blob = b"".join(p[0] for p in parts)
    spans = np.ascontiguousarray(folded[inverse]) if len(raw) else np.zeros((0, 2), np.int64)
    return blob, spans, time.perf_counter() - t0


class TextStore:
    """The folded texts of an index's rows in HBM (proqa_textstore)."""

    def __init__(self, blob, spans):
        """blob: bytes-like of FOLDED text; spans int64 [rows, 2]: first byte and end of each row's text in it."""
        self._lib = _lib.load()
        _lib.require_gpu()
        t0 = time.perf_counter()
        buf = np.frombuffer(blob, dtype=np.uint8) if len(blob) else np.zeros(0, np.uint8)
        spans = np.ascontiguousarray(np.asarray(spans, dtype=np.int64).reshape(-1, 2))
        handle = ctypes.c_void_p()
        _lib.check(self._lib.proqa_textstore_create(buf.ctypes.data if len(buf) else None, len(buf),
                                                    spans.ctypes.data if len(spans) else None, len(spans),
                                                    ctypes.byref(handle)))
        self._h = handle
        self.rows = len(spans)
        self.fold_seconds = 0.0
        self.upload_seconds = time.perf_counter() - t0

    fold = staticmethod(fold)

    @classmethod
    def from_texts(cls, texts):
        """One row per text of the list; identical texts are stored once."""
        t0 = time.perf_counter()
        seen, parts, spans, pos = {}, [], np.zeros((len(texts), 2), np.int64), 0
        for i, text in enumerate(texts):
            span = seen.get(text)
            if span is None:
                b = fold(text)
                parts.append(b)
                span = seen[text] = (pos, pos + len(b))
                pos += len(b)
            spans[i] = span
        fold_seconds = time.perf_counter() - t0
        store = cls(b"".join(parts), spans)
        store.fold_seconds = fold_seconds
        return store

    @classmethod
    def from_sidecar(cls, txt_path, workers=0, pool=None):
        """The rows of a text sidecar.  The fold pass runs on `pool`, or on `workers` processes forked here: call it before
        the process touches the GPU then.  fold_seconds / upload_seconds report what the two parts took."""
        blob, spans, seconds = fold_sidecar(txt_path, workers=workers, pool=pool)
        store = cls(blob, spans)
        store.fold_seconds = seconds
        return store

    def __len__(self):
        return self.rows

    @property
    def device_text_bytes(self):
        n = ctypes.c_int64()
        _lib.check(self._lib.proqa_textstore_info(self._h, None, ctypes.byref(n)))
        return n.value

    def prefilter(self, ids, needles, count=True):
        """ids: int64 CUDA tensor [nq, k] (search_device's I; -1 = empty slot); needles: NeedleTable of the nq questions.
        Returns (mask int32 [nq, ceil(k/32)], count int32 [nq] or None), enqueued on the current stream: bit j % 32 of
        word j // 32 says that ids[q, j] is a row of the store whose folded text passes _may_match for question q."""
        import torch
        if not (ids.is_cuda and ids.dtype == torch.int64 and ids.dim() == 2):
            raise ValueError("prefilter expects an int64 CUDA tensor [nq, k]")
        ids = ids.contiguous()
        nq, k = ids.shape
        mask = torch.empty((nq, (k + 31) // 32), dtype=torch.int32, device=ids.device)
        counts = torch.empty((nq,), dtype=torch.int32, device=ids.device) if count else None
        with torch.cuda.device(ids.device):
            _lib.check(self._lib.proqa_text_prefilter(self._h, needles._h, ids.data_ptr(), nq, k, mask.data_ptr(),
                                                      counts.data_ptr() if count else None, _lib.current_stream_ptr()))
        return mask, counts

    def close(self):
        if self._h:
            _lib.check(self._lib.proqa_textstore_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_needles(questions):
    """[[[token bytes, ...] per alias] per question] -> the six host arrays of proqa_text_needles_create: the distinct
    tokens of each question in order of first use, aliases as indexes into their question's tokens."""
    token_bytes, token_off, q_tok_off = [], [0], [0]
    alias_tokens, alias_off, q_alias_off = [], [0], [0]
    for aliases in questions:
        index = {}
        for alias in aliases:
            for tok in alias:
                if tok not in index:
                    index[tok] = len(index)
                    token_bytes.append(tok)
                    token_off.append(token_off[-1] + len(tok))
                alias_tokens.append(index[tok])
            alias_off.append(len(alias_tokens))
        q_tok_off.append(len(token_off) - 1)
        q_alias_off.append(len(alias_off) - 1)
    return (np.frombuffer(b"".join(token_bytes) + b"\0", dtype=np.uint8), np.asarray(token_off, np.int64),
            np.asarray(q_tok_off, np.int64), np.asarray(alias_tokens + [0], np.int32), np.asarray(alias_off, np.int64),
            np.asarray(q_alias_off, np.int64))


class NeedleTable:
    """The folded needles of a batch of questions on the device (proqa_text_needles): validated, packed and uploaded once."""

    def __init__(self, questions):
        self._lib = _lib.load()
        self.nq = len(questions)
        arrays = pack_needles(questions)
        handle = ctypes.c_void_p()
        _lib.check(self._lib.proqa_text_needles_create(*[a.ctypes.data for a in arrays], self.nq, ctypes.byref(handle)))
        self._h = handle

    def close(self):
        if self._h:
            _lib.check(self._lib.proqa_text_needles_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
