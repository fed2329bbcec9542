"""The reader's training sampler (qa/online_sampler.py of the reference) with the per-question retrieval on the device.

The reference's `OnlineSampler.load` does, per question: the question through the query tower, a faiss search of k = 5000,
I[5000] to the host, 5000 `str()` + dict lookups, 5000 `in gold_paras` tests, a gather of 5000 x 128 rows on the host that
the loop then copies to the GPU as float32, and -- for the top `k` passages only -- text from the DB, answer matching, word and
piece offsets, spans and the padded tensors.  Here everything up to the top-`k` text work is three launches that leave nothing on
the host but a record of (2 + k) int64:

    encode    retriever.get_embed(question, True) under no_grad, in eval() (dropout off: a deterministic retrieval; the
              reference runs the pass in whatever mode the model is in)
    search    IndexFlatIP.search_device(q, 5000): the exact inner-product top 5000 (the reference's IVF index ranks by L2,
              see online_retriever.py; the IVF index here serves k <= 128)
    collect   IndexFlatIP.collect_labeled_device(I, gold rows of the question, head=k): para_embed[I] in the index's dtype,
              top5000_labels as the int32 the loss reads, and the record {rows found, sum of labels, I[:k]}

The gold rows come from the matched file: at construction `index2paraid` is inverted once, every question's `matched_paras`
keys become an ascending array of rows, and all of them are uploaded as one int64 CSR buffer; the questions' token ids go up
there too, as one padded buffer.  Per question the record is the one device-to-host copy and the integer tensors of the batch,
filled into one pinned int64 buffer, are the one host-to-device copy (`net_input` holds views of it).  That count holds for
a retriever whose get_embed takes (check_mask, seq_lens_host) -- BertForRetriever and TrainableRetriever -- and so makes no
host round trip of its own; it is measured in tests/test_reader_sampler_gpu.py, not taken from `transfers`.  The record is
not the only wait for the device: search_device at k = 5000 synchronises its stream inside the library.

The three launches take several questions as they take one (retrieve_many: one tower pass over the right-padded ids, one
search, IndexFlatIP.collect_labeled_multi_device, one copy of the records down), and retrieve is the one-question case.
load(lookahead=...) retrieves in one such step the questions its caller will draw before the retriever's weights can next
change -- the caller says how many -- and yields them one by one.

Host side, for the top `k` passages: qa_utils (char_to_word_offset, orig_to_tok_index, match_answer_span,
find_ans_span_with_char_offsets) over the native WordPiece tokenizer; matched strings are sorted (the reference iterates a
`set`), and prepared passages are cached by row.  An index with fewer than 5000 rows yields the rows it has.  No CPU path.
"""
import collections
import inspect
import json
import random
import time

import numpy as np
import torch

from .basic_tokenizer import SimpleTokenizer
from .index import IndexFlatIP
from .qa_utils import (WordPieces, char_to_word_offset, find_ans_span_with_char_offsets, hash_question, match_answer_span,
                       normalize, orig_to_tok_index, prepare_many)

SEARCH_K = 5000       # qa/online_sampler.py:113
MAX_HEAD = 64         # the record of proqa_sampler_collect_device carries at most 64 ids


def invert_index2paraid(index2paraid):
    """{"<row>": paragraph id} (idx_id.json) or a row-ordered sequence of paragraph ids -> {paragraph id: row}"""
    if isinstance(index2paraid, dict):
        return {pid: int(row) for row, pid in index2paraid.items()}
    return {pid: row for row, pid in enumerate(index2paraid)}


def gold_row_csr(questions, qid2goldparas, paraid2row):
    """questions: the question strings of the training data -> (rows int64 [total], offsets int64 [n + 1], {qid: slot}):
    the rows of every question's matched paragraphs, ascending within a question (a paragraph id that names no row of the
    index is dropped; a question asked twice shares one slot).  A question without an entry in the matched file is a
    ValueError here -- the reference dies with a KeyError in the middle of the epoch."""
    slots, chunks, offsets = {}, [], [0]
    for question in questions:
        qid = hash_question(question)
        if qid in slots:
            continue
        if qid not in qid2goldparas:
            raise ValueError(f"training question {question!r} has no entry in the matched-paragraph file")
        rows = sorted({paraid2row[p] for p in qid2goldparas[qid] if p in paraid2row})
        slots[qid] = len(chunks)
        chunks.append(np.asarray(rows, dtype=np.int64))
        offsets.append(offsets[-1] + len(rows))
    rows = np.concatenate(chunks) if chunks else np.empty(0, dtype=np.int64)
    return rows.astype(np.int64), np.asarray(offsets, dtype=np.int64), slots


def prepare_passages(texts, wordpieces):
    """prepare() of normalised passages (qa/prepro_utils.py:150-175), all words WordPiece'd in one batch: prepare_many's
    dicts plus text, char_to_word_offset and orig_to_tok_index"""
    out = prepare_many(texts, wordpieces)
    for p, prep in zip(texts, out):
        prep["text"] = p
        prep["char_to_word_offset"] = np.asarray(char_to_word_offset(p), dtype=np.int32)      # 4 bytes per character
        prep["orig_to_tok_index"] = orig_to_tok_index(prep["tok_to_orig_index"], len(prep["doc_tokens"]))
    return out


def passage_spans(prep, answers, basic_tokenizer, tokenize, regex=False):
    """(covered by the match, starts, ends) of one prepared passage, in pieces of the whole passage
    (online_sampler.py:133-164); the matched strings in sorted order"""
    p = prep["text"]
    matched = match_answer_span(p, answers, basic_tokenizer, match="regex" if regex else "string")
    starts, ends = [], []
    for s in matched:
        char_starts = [i for i in range(len(p)) if p.startswith(s, i)]
        if not char_starts:
            continue
        answer = {"text": s, "char_spans": [(c, c + len(s) - 1) for c in char_starts]}
        for a, b in find_ans_span_with_char_offsets(answer, prep["char_to_word_offset"], prep["doc_tokens"],
                                                    prep["all_doc_tokens"], prep["orig_to_tok_index"], tokenize):
            starts.append(a)
            ends.append(b)
    return int(len(matched) > 0), starts, ends


def span_positions(n_kept, para_offset, covered, starts, ends):
    """(start positions, end positions, covered) of a passage cut to n_kept pieces, in positions of the joined sequence
    (online_sampler.py:232-252): a span that starts past the cut is dropped, one that ends past it is clipped; ([-1], [-1], 0)
    when none is left"""
    st, en = [], []
    if covered:
        for s, e in zip(starts, ends):
            assert s <= e
            if s >= n_kept:
                continue
            st.append(min(s, n_kept - 1) + para_offset)
            en.append(min(e, n_kept - 1) + para_offset)
    return st or [-1], en or [-1], int(len(st) > 0)


class OnlineSampler:
    def __init__(self, raw_data, tokenizer, max_query_length, max_length, db, para_embed=None,
                 index2paraid="retrieval/index_data/idx_id.json", matched_para_path="", exact_search=False, cased=False,
                 regex=False, index=None, device=None, cache_passages=16384):
        """The reference's arguments (exact_search is accepted and has no effect: the search is exact), plus `index`: an
        IndexFlatIP that already holds the rows (para_embed may then be None).  para_embed: [N, 128] float16 / float32
        array, or the IndexFlatIP itself.  index2paraid: a path to idx_id.json, its dict, or a row-ordered sequence.
        cache_passages: prepared passages kept (least recently used dropped first; a passage of 400 words holds ~30 KB)."""
        if cased:
            raise ValueError("OnlineSampler: cased (--use-spanbert) tokenization is not built")
        if matched_para_path == "":
            raise ValueError("OnlineSampler: matched_para_path is required (the reference's load() reads qid2goldparas, "
                             "which exists only with it)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.max_length, self.max_query_length = int(max_length), int(max_query_length)
        self.cased, self.regex = False, bool(regex)
        self.tokenizer = tokenizer
        self.para_db = db
        if isinstance(para_embed, IndexFlatIP):
            index, para_embed = para_embed, None
        if index is None:
            if para_embed is None:
                raise ValueError("OnlineSampler needs para_embed or an index")
            para_embed = np.ascontiguousarray(para_embed)
            with torch.cuda.device(self.device):      # proqa_index_create binds the index to the current device
                index = IndexFlatIP(128, capacity=para_embed.shape[0])
                step = 1 << 21
                for r0 in range(0, para_embed.shape[0], step):
                    index.add(para_embed[r0:r0 + step])
        elif not isinstance(index, IndexFlatIP):
            raise ValueError("OnlineSampler searches k = 5000 on the exact IndexFlatIP (the IVF index serves k <= 128)")
        self.index = index
        with open(raw_data) as f:
            self.qa_data = [json.loads(l) for l in f.readlines()]
        self._file_data = list(self.qa_data)          # the file's order; qa_data is _file_data in the order of _order
        self._order = list(range(len(self.qa_data)))
        if isinstance(index2paraid, str):
            with open(index2paraid) as f:
                index2paraid = json.load(f)
        self.index2paraid = index2paraid
        self._row2paraid = (lambda r: index2paraid[str(r)]) if isinstance(index2paraid, dict) else index2paraid.__getitem__
        self.matched_para_path = matched_para_path
        print(f"Load matched gold paras from {matched_para_path}")
        with open(matched_para_path) as f:
            annotated = [json.loads(l) for l in f.readlines()]
        self.qid2goldparas = {hash_question(item["question"]): item["matched_paras"] for item in annotated}
        rows, self._gold_offsets, self._gold_slot = gold_row_csr([qa["question"] for qa in self.qa_data], self.qid2goldparas,
                                                                 invert_index2paraid(index2paraid))
        self._gold_rows = torch.from_numpy(rows).to(self.device)          # one upload, at construction
        # the questions' token ids, too: one padded int64 buffer, a row per gold slot, so that a question's encode
        # reads a view of it and copies nothing up
        self._q_ids = [None] * len(self._gold_slot)
        for qa in self.qa_data:
            slot = self._gold_slot[hash_question(qa["question"])]
            if self._q_ids[slot] is None:
                self._q_ids[slot] = tokenizer.encode(qa["question"], max_length=self.max_query_length, truncation=True)
        width = max((len(t) for t in self._q_ids), default=1)
        padded = np.zeros((len(self._q_ids), width), dtype=np.int64)
        for slot, t in enumerate(self._q_ids):
            padded[slot, :len(t)] = t
        self._q_ids_dev = torch.from_numpy(padded).to(self.device)
        # and their masks (a prefix of ones per row), for the sampling step of several questions of different lengths
        lengths = np.asarray([len(t) for t in self._q_ids], dtype=np.int64).reshape(-1, 1)
        self._q_mask_dev = torch.from_numpy(np.arange(width, dtype=np.int64)[None, :] < lengths).to(self.device)
        self._host_lens = {}       # id(retriever) -> its get_embed takes (check_mask, seq_lens_host)
        self.basic_tokenizer = SimpleTokenizer()
        self.wordpieces = WordPieces(tokenizer)
        self._cls, self._sep = tokenizer.vocab["[CLS]"], tokenizer.vocab["[SEP]"]
        self._passages = collections.OrderedDict()        # row -> prepared passage, least recently used first
        self.cache_passages = max(int(cache_passages), MAX_HEAD)
        self._answer_pieces = {}   # matched string -> its WordPiece tokens
        self._pinned = None
        self._pinned_copied = None     # event behind the last copy out of _pinned
        self.sync_stages = False   # True: a device synchronise after every stage, so that `seconds` splits device time too
        self.transfers = {"d2h": 0, "h2d": 0}      # the copies this module issues; the tests count the real ones in a profile
        self.seconds = {"encode": 0.0, "search_collect": 0.0, "host_text": 0.0, "h2d": 0.0}
        self.questions_seen = 0
        self.groups = 0            # sampling steps (retrieve_many calls): each is one tower pass, search, collect and record

    def shuffle(self):
        # the same draws from `random` and the same arrangement as random.shuffle(self.qa_data): shuffle() swaps by
        # position, whatever the list holds
        random.shuffle(self._order)
        self.qa_data = [self._file_data[i] for i in self._order]

    def permutation(self):
        """the current order of the questions, as indices into the file's order (what a trainer state saves)"""
        return list(self._order)

    def set_permutation(self, order):
        """put a saved permutation() back; later shuffle() calls continue from it"""
        order = [int(i) for i in order]
        if sorted(order) != list(range(len(self._file_data))):
            raise ValueError("OnlineSampler.set_permutation: not a permutation of the file's questions")
        self._order = order
        self.qa_data = [self._file_data[i] for i in order]

    def __len__(self):
        return len(self.qa_data)

    # -- host side ---------------------------------------------------------------------------------------------------
    def _prepared(self, rows):
        """the prepared passages of `rows` (cached by row): text, words, offsets, pieces"""
        missing = [r for r in dict.fromkeys(rows) if r not in self._passages]
        if missing:
            texts = [normalize(self.para_db.get_doc_text(self._row2paraid(r))) for r in missing]
            for r, prep in zip(missing, prepare_passages(texts, self.wordpieces)):
                self._passages[r] = prep
        out = [self._passages[r] for r in rows]
        for r in rows:
            self._passages.move_to_end(r)
        while len(self._passages) > self.cache_passages:
            self._passages.popitem(last=False)
        return out

    def _tokenize_answer(self, text):
        pieces = self._answer_pieces.get(text)
        if pieces is None:
            pieces = self._answer_pieces[text] = self.tokenizer.tokenize(text)
        return pieces

    def _spans(self, prep, answers):
        return passage_spans(prep, answers, self.basic_tokenizer, self._tokenize_answer, self.regex)

    def _pinned_buffer(self, n):
        # the buffer is written again only once its last copy up has run: within a group of load(lookahead=...) no
        # record copy stands between two batches to wait for it
        if self._pinned_copied is not None:
            self._pinned_copied.synchronize()
        if self._pinned is None or self._pinned.numel() < n:
            self._pinned = torch.empty(max(n, 1 << 14), dtype=torch.int64).pin_memory()
        return self._pinned[:n]

    def _collate(self, qa, q_ids, preps, spans):
        """online_sampler.py:199-262, 355-388: the integer tensors of one batch in one pinned buffer, one copy up"""
        B, Lq = len(preps), len(q_ids)
        para_offset = Lq
        keep = [min(len(p["piece_ids"]), max(0, self.max_length - para_offset - 1)) for p in preps]
        L = max(Lq + n + 1 for n in keep)
        positions = [span_positions(n, para_offset, *sp) for n, sp in zip(keep, spans)]
        S = max(len(st) for st, _, _ in positions)
        sizes = [B * L] * 4 + [B * S] * 2 + [B] + [B * Lq] * 2
        flat = self._pinned_buffer(sum(sizes))
        host = flat.numpy()
        parts, at = [], 0
        for n, shape in zip(sizes, [(B, L)] * 4 + [(B, S)] * 2 + [(B, 1)] + [(B, Lq)] * 2):
            parts.append(host[at:at + n].reshape(shape))
            at += n
        ids, seg, pmask, imask, start, end, target, ids_q, mask_q = parts
        for a in (ids, seg, pmask, imask):
            a.fill(0)
        start.fill(-1)
        end.fill(-1)
        q_inner = list(q_ids[1:-1])
        for b, (p, n) in enumerate(zip(preps, keep)):
            row = [self._cls] + q_inner + [self._sep] + p["piece_ids"][:n] + [self._sep]
            ids[b, :len(row)] = row
            seg[b, Lq:len(row)] = 1
            pmask[b, para_offset:len(row) - 1] = 1
            imask[b, :len(row)] = 1
            st, en, covered = positions[b]
            start[b, :len(st)] = st
            end[b, :len(en)] = en
            target[b, 0] = covered
        ids_q[:] = np.asarray(q_ids, dtype=np.int64)[None]
        mask_q.fill(1)
        t0 = time.perf_counter()
        dev = torch.empty(flat.numel(), dtype=torch.int64, device=self.device)
        dev.copy_(flat, non_blocking=True)          # the one host-to-device copy of the batch
        self.transfers["h2d"] += 1
        if self._pinned_copied is None:
            self._pinned_copied = torch.cuda.Event()
        self._pinned_copied.record(torch.cuda.current_stream(self.device))
        if self.sync_stages:
            torch.cuda.current_stream(self.device).synchronize()
        self.seconds["h2d"] += time.perf_counter() - t0
        views, at = [], 0
        for n, shape in zip(sizes, [(B, L)] * 4 + [(B, S)] * 2 + [(B, 1)] + [(B, Lq)] * 2):
            views.append(dev[at:at + n].view(shape))
            at += n
        names = ("input_ids", "segment_ids", "paragraph_mask", "input_mask", "start_positions", "end_positions",
                 "para_targets", "input_ids_q", "input_mask_q")
        net_input = dict(zip(names, views))
        net_input["paragraph_mask"] = net_input["paragraph_mask"].bool()       # the reference's dtype (a device cast)
        qid = hash_question(qa["question"])
        return {"id": [qid] * B, "q": [qa["question"]] * B,
                "wp_tokens": [p["all_doc_tokens"] for p in preps], "para_offset": [para_offset] * B,
                "true_answers": [qa["answer"]] * B, "net_input": net_input}

    # -- the sampler ---------------------------------------------------------------------------------------------------
    def retrieve(self, retriever, question, head):
        """encode + search + collect of one question -> (q_ids, para_embed [n_live, 128], labels int32 [n_live],
        n_live, sum of labels, the first min(head, n_live) rows as a list).  The record is this method's one device-to-host
        copy.  It is retrieve_many of that one question."""
        return self.retrieve_many(retriever, [question], head)[0]

    def retrieve_many(self, retriever, questions, head):
        """encode + search + collect of several questions in ONE sampling step -- one pass of the question tower over their
        right-padded token ids, one search_device, one collect_labeled_multi_device, one copy of the records to the host --
        -> [retrieve's tuple for every question]; para_embed and labels are views into the step's buffers.  The questions
        are retrieved with the weights the retriever holds now, so the caller groups only questions between which no weight
        changes.  A question may occur twice (both read one gold slot)."""
        t0 = time.perf_counter()
        if not questions:
            return []
        slots = [self._gold_slot.get(hash_question(question)) for question in questions]
        for slot, question in zip(slots, questions):
            if slot is None:
                raise ValueError(f"question {question!r} is not one of the sampler's training questions")
        q_ids = [self._q_ids[slot] for slot in slots]
        lens = [len(t) for t in q_ids]
        width = max(lens)
        with torch.no_grad():
            # uploaded at construction: nothing goes up here.  A row is zero past its question, so rows cut to the longest
            # question are right-padded
            ids = torch.cat([self._q_ids_dev[slot:slot + 1, :width] for slot in slots])
            mask = torch.cat([self._q_mask_dev[slot:slot + 1, :width] for slot in slots])
            takes_lens = self._host_lens.get(id(retriever))
            if takes_lens is None:
                params = inspect.signature(retriever.get_embed).parameters
                takes_lens = self._host_lens[id(retriever)] = "seq_lens_host" in params and "check_mask" in params
            # the mask is a prefix of ones per row and the lengths are known here: a tower that takes host lengths makes
            # no host round trip
            extra = {"check_mask": False, "seq_lens_host": lens} if takes_lens else {}
            was_training = bool(getattr(retriever, "training", False))
            if was_training:
                retriever.eval()
            try:
                q = retriever.get_embed({"input_ids": ids, "input_mask": mask}, True, **extra)["embed"]
            finally:
                if was_training:
                    retriever.train()
        q = q.reshape(len(slots), -1)
        if self.sync_stages:
            torch.cuda.current_stream(self.device).synchronize()
        t1 = time.perf_counter()
        _, I = self.index.search_device(q, SEARCH_K)
        begin = [int(self._gold_offsets[slot]) for slot in slots]
        count = [int(self._gold_offsets[slot + 1]) - b for slot, b in zip(slots, begin)]
        dtype = torch.float32 if self.index.exact_f32 else torch.float16
        rows, labels, records = self.index.collect_labeled_multi_device(
            I, self._gold_rows if self._gold_rows.numel() else None, begin, count, head, dtype)
        records = records.cpu().tolist()            # the one device-to-host copy of the sampling step (it synchronises)
        self.transfers["d2h"] += 1
        self.groups += 1
        t2 = time.perf_counter()
        self.seconds["encode"] += t1 - t0
        self.seconds["search_collect"] += t2 - t1
        out = []
        for i, record in enumerate(records):
            n_live, n_gold = record[0], record[1]
            out.append((q_ids[i], rows[i, :n_live], labels[i, :n_live], n_live, n_gold, [r for r in record[2:] if r >= 0]))
        return out

    def _batch(self, qa, retrieved):
        """the host text work of one retrieved question: {} when neither its top 5000 nor its top k passages carry the
        answer, else the reference's batch with the tensors of net_input on the device"""
        q_ids, para_embed, labels, n_live, n_gold, top_rows = retrieved
        t0 = time.perf_counter()
        preps = self._prepared(top_rows)
        spans = [self._spans(p, qa["answer"]) for p in preps]
        if not preps or (n_gold == 0 and not any(c for c, _, _ in spans)):
            self.seconds["host_text"] += time.perf_counter() - t0
            return {}
        h2d_before = self.seconds["h2d"]
        batch = self._collate(qa, q_ids, preps, spans)
        self.seconds["host_text"] += time.perf_counter() - t0 - (self.seconds["h2d"] - h2d_before)
        batch["net_input"]["para_embed"] = para_embed
        batch["net_input"]["top5000_labels"] = labels
        return batch

    def load(self, retriever, k=5, start=0, lookahead=None):
        """Yields, per question, {} when neither its top 5000 nor its top k passages carry the answer, else the
        reference's batch with the tensors of net_input on the device.  start: the first `start` questions of the current
        order are left out (a resumed epoch).  lookahead: None retrieves question by question; else a callable that returns
        how many questions, counting the next one, will be drawn before the retriever's weights can next change.  It is asked
        whenever every retrieved question has been yielded; that many questions (at most what the epoch still holds) are
        then retrieved in one retrieve_many and yielded one by one, para_embed and top5000_labels being views into the
        group's buffers."""
        if not 0 < k <= MAX_HEAD:
            raise ValueError(f"OnlineSampler.load: k must be in [1, {MAX_HEAD}], got {k}")
        if not 0 <= start <= len(self.qa_data):
            raise ValueError(f"OnlineSampler.load: start must be in [0, {len(self.qa_data)}], got {start}")
        todo = self.qa_data[start:] if start else self.qa_data
        if lookahead is None:
            for qa in todo:
                self.questions_seen += 1
                yield self._batch(qa, self.retrieve(retriever, qa["question"], k))
            return
        at = 0
        while at < len(todo):
            n = int(lookahead())
            if n < 1:
                raise ValueError(f"OnlineSampler.load: lookahead() must return at least 1, got {n}")
            group = todo[at:at + n]
            at += len(group)
            for qa, retrieved in zip(group, self.retrieve_many(retriever, [qa["question"] for qa in group], k)):
                self.questions_seen += 1
                yield self._batch(qa, retrieved)
