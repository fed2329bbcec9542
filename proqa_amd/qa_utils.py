"""Host side of the reader's --do_predict (qa/train_retrieve_qa.py): pair building, answer text, EM metric, alpha sweep.

Written for this project and pinned to the reference's behaviour by tests/golden/reader_golden.json:
    prepare             qa/prepro_utils.py:150-175 (words split on whitespace, each word WordPiece'd on its own)
    build_pair          qa/online_sampler.py:285-335 ([CLS] q [SEP] p [SEP], segments, paragraph mask, para_offset)
    get_final_text      qa/eval_utils.py:15-83 (the WordPiece answer projected back onto the original words)
    normalize_answer, exact_match_score, regex_match_score, metric_max_over_ground_truths   qa/official_eval.py
    hash_question       qa/prepro_utils.py:12-14
    alpha_sweep         qa/train_retrieve_qa.py:365-397
marginal_answers (answer probabilities summed over the n-best spans of a question's passages) is not in the reference: it
is the decoding rule its training objective implies.
"""
import ctypes
import hashlib
import json
import re
import string
import unicodedata

import numpy as np

ALPHAS = [0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.5, 0.55, 0.6, 0.7, 0.8, 0.9, 1]


def hash_question(q):
    return hashlib.md5(q.encode()).hexdigest()


def normalize(text):
    return unicodedata.normalize("NFD", text)


def _is_space(ch):
    """The passage word separator: space, tab, newline, carriage return, or any Unicode space separator (Zs)."""
    return ch in " \t\n\r" or unicodedata.category(ch) == "Zs"


def split_words(text):
    """Maximal runs of non-separator characters, in order."""
    words, cur = [], []
    for ch in text:
        if _is_space(ch):
            if cur:
                words.append("".join(cur))
                cur = []
        else:
            cur.append(ch)
    if cur:
        words.append("".join(cur))
    return words


# ---- pair building -----------------------------------------------------------------------------------------------

class WordPieces:
    """WordPiece of single words, many at a time: the words go through libproqa_hip.so's own tokenizer
    (proqa_wordpiece_encode_batch, via TokenizeCollate's vocabulary check) in large batches; a word it declines, or any
    word when the tokenizer is not a plain BERT WordPiece one, goes through tokenizer.tokenize."""

    _NATIVE_MAX_CHARS = 62     # a word of n characters has at most n pieces: [CLS] + 62 + [SEP] fit 64 slots

    def __init__(self, tokenizer, threads=8):
        from .datasets import TokenizeCollate
        self.tokenizer = tokenizer
        self.collate = TokenizeCollate(tokenizer, self._NATIVE_MAX_CHARS + 2, native_threads=max(1, int(threads)))
        self.native = self.collate.has_native
        vocab = tokenizer.get_vocab()
        self.id_to_tok = [None] * (max(vocab.values()) + 1)
        for t, i in vocab.items():
            self.id_to_tok[i] = t

    def _python(self, word):
        pieces = self.tokenizer.tokenize(word)
        return pieces, self.tokenizer.convert_tokens_to_ids(pieces)

    def __call__(self, words, chunk=1 << 17):
        """words -> (pieces: list of lists of str, ids: list of lists of int), word by word."""
        out_p, out_i = [None] * len(words), [None] * len(words)
        native_rows = []
        for n, w in enumerate(words):
            if self.native and len(w) <= self._NATIVE_MAX_CHARS:
                native_rows.append(n)
            else:
                out_p[n], out_i[n] = self._python(w)
        for c0 in range(0, len(native_rows), chunk):
            rows = native_rows[c0:c0 + chunk]
            lib, h = self.collate.native_handle()
            from . import _lib
            raw = [words[n].encode("utf-8") for n in rows]
            m, L = len(rows), self._NATIVE_MAX_CHARS + 2
            ptrs = (ctypes.c_char_p * m)(*raw)
            sizes = np.fromiter(map(len, raw), dtype=np.int64, count=m)
            ids = np.empty((m, L), dtype=np.int64)
            lens = np.empty(m, dtype=np.int32)
            _lib.check(lib.proqa_wordpiece_encode_batch(h, ptrs, sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), m, L,
                                                        ids.ctypes.data, lens.ctypes.data, self.collate.native_threads))
            id_rows = ids.tolist()
            for k, n in enumerate(rows):
                ln = int(lens[k])
                if ln < 0 or ln >= L:      # declined (-1), or possibly truncated: the tokenizer itself
                    out_p[n], out_i[n] = self._python(words[n])
                else:
                    piece_ids = id_rows[k][1:ln - 1]
                    out_i[n] = piece_ids
                    out_p[n] = [self.id_to_tok[i] for i in piece_ids]
        return out_p, out_i


def prepare_many(passages, wordpieces):
    """prepare() of every passage, with all their words WordPiece'd in one batch.

    Returns a list of dicts: doc_tokens (words), tok_to_orig_index, all_doc_tokens (pieces), piece_ids."""
    words_of = [split_words(p) for p in passages]
    flat = [w for ws in words_of for w in ws]
    pieces, ids = wordpieces(flat)
    out, k = [], 0
    for ws in words_of:
        t2o, toks, tids = [], [], []
        for i in range(len(ws)):
            toks.extend(pieces[k])
            tids.extend(ids[k])
            t2o.extend([i] * len(pieces[k]))
            k += 1
        out.append({"doc_tokens": ws, "tok_to_orig_index": t2o, "all_doc_tokens": toks, "piece_ids": tids})
    return out


def char_to_word_offset(text):
    """prepare()'s char_to_word_offset (qa/prepro_utils.py:150-164): for every character of text the index of the word of
    split_words(text) it belongs to; a separator belongs to the word before it (-1 before the first word)."""
    out, n, inside = [], 0, False
    for ch in text:
        if _is_space(ch):
            inside = False
        elif not inside:
            n += 1
            inside = True
        out.append(n - 1)
    return out


def orig_to_tok_index(tok_to_orig_index, n_words):
    """prepare()'s orig_to_tok_index from its inverse: the position of every word's first piece among all pieces (a word
    without pieces gets the position of the next word's first piece, as the reference's running length gives it)."""
    out, k = [], 0
    for w in range(n_words):
        while k < len(tok_to_orig_index) and tok_to_orig_index[k] < w:
            k += 1
        out.append(k)
    return out


def match_answer_span(p, answer, tokenizer, match="string"):
    """The strings of the (normalised) passage p that match the answers (qa/prepro_dense.py:30-42, 57-74), SORTED -- the
    reference returns them in `set` order, which changes from run to run.  string: every run of the SimpleTokenizer's
    tokens of p whose lower-cased text equals an answer's, as the passage spells it; regex: every match of answer[0]."""
    if match == "string":
        tokens = tokenizer.tokenize(p)
        text = tokens.words(uncased=True)
        matched = set()
        for single in answer:
            single = tokenizer.tokenize(normalize(single)).words(uncased=True)
            for i in range(0, len(text) - len(single) + 1):
                if single == text[i:i + len(single)]:
                    matched.add(tokens.slice(i, i + len(single)).untokenize())
        return sorted(matched)
    if match == "regex":
        pattern = normalize(answer[0])
        try:
            compiled = re.compile(pattern, flags=re.IGNORECASE + re.UNICODE + re.MULTILINE)
        except BaseException:
            print("Regular expression failed to compile: %s" % pattern)
            return []
        return sorted({m.group() for m in re.finditer(compiled, p)})
    raise ValueError(f"match must be 'string' or 'regex', got {match!r}")


def _improve_answer_span(all_doc_tokens, input_start, input_end, tok_answer_text):
    """The narrowest run of pieces inside [input_start, input_end] that spells the tokenised answer, leftmost start first
    and longest end first (qa/prepro_utils.py:62-72); the input span when there is none."""
    for new_start in range(input_start, input_end + 1):
        for new_end in range(input_end, new_start - 1, -1):
            if " ".join(all_doc_tokens[new_start:new_end + 1]) == tok_answer_text:
                return new_start, new_end
    return input_start, input_end


def find_ans_span_with_char_offsets(detected_ans, char_to_word, doc_tokens, all_doc_tokens, orig_to_tok, tokenize):
    """detected_ans = {"text", "char_spans": [(first char, LAST char)]} -> [(first piece, last piece)] per char span
    (qa/prepro_utils.py:74-99): the pieces of the words the characters lie in, narrowed to the pieces that spell the
    answer.  tokenize: text -> WordPiece tokens (the tokenizer's own `tokenize`).  The reference's "Could not find answer"
    print is left out."""
    tok_answer_text = " ".join(tokenize(detected_ans["text"]))
    spans = []
    for char_start, char_end in detected_ans["char_spans"]:
        tok_start, tok_end = char_to_word[char_start], char_to_word[char_end]
        sub_start = orig_to_tok[tok_start]
        sub_end = orig_to_tok[tok_end + 1] - 1 if tok_end < len(doc_tokens) - 1 else len(all_doc_tokens) - 1
        spans.append(_improve_answer_span(all_doc_tokens, sub_start, sub_end, tok_answer_text))
    return spans


def build_pair(q_ids, p_ids, max_seq_length, cls_id, sep_id):
    """q_ids = tokenizer.encode(question) ([CLS] ... [SEP]), p_ids = the passage's piece ids ->
    (input_ids, segment_ids, para_offset, n_passage_pieces_kept).  The passage is cut to max_seq_length - para_offset - 1
    pieces; segment 0 runs up to and including the first [SEP]; the paragraph mask is [para_offset, len - 1)."""
    para_offset = len(q_ids)
    keep = max(0, min(len(p_ids), max_seq_length - para_offset - 1))
    q_inner = list(q_ids[1:-1])
    ids = [cls_id] + q_inner + [sep_id] + list(p_ids[:keep]) + [sep_id]
    seg = [0] * (len(q_inner) + 2) + [1] * (keep + 1)
    return ids, seg, para_offset, keep


# ---- answer text --------------------------------------------------------------------------------------------------

def _is_punct(ch):
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


def _is_ctrl(ch):
    if ch in "\t\n\r":
        return False
    return unicodedata.category(ch).startswith("C")


def basic_tokenize(text, do_lower_case=True):
    """BERT's basic tokenizer as the reference's eval_utils uses it (qa/tokenizer.py: no CJK splitting)."""
    cleaned = []
    for ch in text:
        if ord(ch) in (0, 0xFFFD) or _is_ctrl(ch):
            continue
        cleaned.append(" " if _is_space(ch) else ch)
    out = []
    for tok in "".join(cleaned).split():
        if do_lower_case:
            tok = "".join(c for c in unicodedata.normalize("NFD", tok.lower()) if unicodedata.category(c) != "Mn")
        cur = ""
        for ch in tok:
            if _is_punct(ch):
                if cur:
                    out.append(cur)
                    cur = ""
                out.append(ch)
            else:
                cur += ch
        if cur:
            out.append(cur)
    return " ".join(out).split()


def _without_spaces(text):
    """(text without ' ' characters, {index in that string: index in text})"""
    chars, where = [], {}
    for i, ch in enumerate(text):
        if ch == " ":
            continue
        where[len(chars)] = i
        chars.append(ch)
    return "".join(chars), where


def get_final_text(pred_text, orig_text, do_lower_case=True):
    """The part of orig_text (words joined by ' ') that the WordPiece text pred_text covers; orig_text itself when the
    character alignment between the basic-tokenised words and the original does not hold."""
    tok_text = " ".join(basic_tokenize(orig_text, do_lower_case))
    start = tok_text.find(pred_text)
    if start == -1:
        return orig_text
    end = start + len(pred_text) - 1
    orig_ns, orig_map = _without_spaces(orig_text)
    tok_ns, tok_map = _without_spaces(tok_text)
    if len(orig_ns) != len(tok_ns):
        return orig_text
    tok_to_ns = {s: ns for ns, s in tok_map.items()}
    if start not in tok_to_ns or tok_to_ns[start] not in orig_map:
        return orig_text
    if end not in tok_to_ns or tok_to_ns[end] not in orig_map:
        return orig_text
    return orig_text[orig_map[tok_to_ns[start]]:orig_map[tok_to_ns[end]] + 1]


def answer_text(start, end, para_offset, doc_tokens, wp_tokens, tok_to_orig_index, do_lower_case=True):
    """Text of the span [start, end] (positions in the sequence, as the span kernel returns them); "" when there is
    no span (start < 0: a passage without any paragraph token)."""
    if start < 0:
        return ""
    s, e = start - para_offset, end - para_offset
    orig_tokens = doc_tokens[tok_to_orig_index[s]:tok_to_orig_index[e] + 1]
    tok_text = " ".join(wp_tokens[s:e + 1]).replace(" ##", "").replace("##", "").strip()
    tok_text = " ".join(tok_text.split())
    return get_final_text(tok_text, " ".join(orig_tokens), do_lower_case)


# ---- metric -------------------------------------------------------------------------------------------------------

_PUNCT = set(string.punctuation)


def normalize_answer(s):
    s = "".join(ch for ch in s.lower() if ch not in _PUNCT)
    s = re.sub(r"\b(a|an|the)\b", " ", s)
    return " ".join(s.split())


def exact_match_score(prediction, ground_truth):
    return normalize_answer(prediction) == normalize_answer(ground_truth)


def regex_match_score(prediction, pattern):
    try:
        compiled = re.compile(pattern, flags=re.IGNORECASE + re.UNICODE + re.MULTILINE)
    except BaseException:
        print("Regular expression failed to compile: %s" % pattern)
        return False
    return compiled.match(prediction) is not None


def metric_max_over_ground_truths(metric_fn, prediction, ground_truths):
    return max(metric_fn(prediction, g) for g in ground_truths)


# ---- alpha sweep --------------------------------------------------------------------------------------------------

def sweep_key(alpha):
    """Sort key of one alpha: alpha * span + (1 - alpha) * rank, descending.  An entry without a span (span_score None: a
    passage without any paragraph token, which the reference cannot evaluate at all) ranks below every entry that has one,
    at every alpha -- a -inf span score would make the key NaN at alpha 0 and NaN keys break the order of the whole list."""
    def key(x):
        if x["span_score"] is None:
            return (0, 0.0)
        return (1, alpha * x["span_score"] + (1 - alpha) * x["rank_score"])
    return key


def alpha_sweep(qid2results, qid2ground, regex=False, save_prefix=None, out=print):
    """qid2results: {qid: [dict(text, rank_score, span_score, passage, question), ...]} in retrieval order (insertion
    order of the questions is kept); span_score None = no span.  For each alpha the list of every question is re-sorted --
    stably, starting from the previous alpha's order, as the reference sorts in place -- by sweep_key(alpha); the top
    entry is scored.  Prints the reference's two lines per alpha; returns ([(alpha, em)], best em)."""
    match_fn = regex_match_score if regex else exact_match_score
    res, best = [], 0
    for alpha in ALPHAS:
        saved, ems = [], []
        for qid in qid2results:
            qid2results[qid] = sorted(qid2results[qid], key=sweep_key(alpha), reverse=True)
            top = qid2results[qid][0]
            ems.append(metric_max_over_ground_truths(match_fn, top["text"], qid2ground[qid]))
            saved.append({"question": top["question"], "para": top["passage"], "answer": top["text"],
                          "rank_score": top["rank_score"], "gold": qid2ground[qid], "em": ems[-1]})
        em = np.mean(ems)
        if em > best:
            best = em
        out(f"evaluated {len(ems)} examples...")
        out(f"alpha: {alpha}; avg. EM: {em}")
        res.append((alpha, em))
        if save_prefix:
            with open(f"{save_prefix}_{alpha}.json", "w") as g:
                for line in saved:
                    g.write(json.dumps(line) + "\n")
    return res, best


# ---- marginal decoding over n-best spans --------------------------------------------------------------------------

def _logsumexp(xs):
    """float64 log-sum-exp of a list; -inf for an empty list or one of -inf only"""
    m = max(xs, default=-np.inf)
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.sum(np.exp(np.asarray(xs, np.float64) - m))))


def marginal_answers(results, norm="shared"):
    """The decoding rule of the training objective (proqa_reader_loss_f16): the probability of an answer is the sum over
    its mentions, across the passages of one question, of exp(l), l = span score - Z + log r_b.

    results: the question's passages in retrieval order, each dict(rank_score: d_b, lse: (Z^s_b, Z^e_b), candidates:
    [(text, score), ...] in n-best order).  log r_b is the log-softmax of the rank scores over these passages.  norm
    "passage": Z = Z^s_b + Z^e_b, every passage normalised on its own; "shared": Z = logsumexp_b Z^s_b + logsumexp_b Z^e_b,
    the shared norm of training over the question's sequences.  Everything in float64.

    Returns [dict(key, prob, text)] sorted by prob descending: key = normalize_answer(text), text that of the key's first
    mention in (passage, n) order, which also breaks ties.  Mentions with empty text are dropped unless there is nothing
    else; a mention whose l is NaN (overflowed logits) is dropped."""
    if norm not in ("shared", "passage"):
        raise ValueError(f"norm must be 'shared' or 'passage', got {norm!r}")
    if not results:
        return []
    log_r = np.asarray([x["rank_score"] for x in results], np.float64)
    log_r = log_r - _logsumexp(log_r.tolist())
    shared = _logsumexp([float(x["lse"][0]) for x in results]) + _logsumexp([float(x["lse"][1]) for x in results])
    mentions = []       # (text, l) in (passage, n) order
    with np.errstate(invalid="ignore", over="ignore"):
        for b, x in enumerate(results):
            z = shared if norm == "shared" else float(x["lse"][0]) + float(x["lse"][1])
            for text, score in x["candidates"]:
                l = np.float64(score) - z + log_r[b]
                if not np.isnan(l):
                    mentions.append((text, l))
        mentions = [m for m in mentions if m[0].strip()] or mentions
        order, prob, first = [], {}, {}
        for text, l in mentions:
            key = normalize_answer(text)
            if key not in prob:
                order.append(key)
                prob[key], first[key] = 0.0, text
            prob[key] += float(np.exp(l))
    rank = {k: n for n, k in enumerate(order)}
    return [{"key": k, "prob": prob[k], "text": first[k]} for k in sorted(order, key=lambda k: (-prob[k], rank[k]))]
