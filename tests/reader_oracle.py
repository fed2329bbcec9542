"""NumPy restatements the reader tests compare against (helpers, not tests)."""
import numpy as np

from oracle import bert_oracle


def typed_tower(sd, prefix, input_ids, segment_ids, input_mask, n_layers, n_heads, eps=1e-12):
    """(last hidden [B, S, H], pooled [B, H]) of a BertModel WITH token types, from the oracle's type-0 tower: the word
    table is widened to [word; word + type1 - type0] and segment-1 tokens read the second half."""
    e = prefix + ".embeddings."
    word = np.asarray(sd[e + "word_embeddings.weight"], np.float32)
    types = np.asarray(sd[e + "token_type_embeddings.weight"], np.float32)
    sd2 = dict(sd)
    sd2[e + "word_embeddings.weight"] = np.concatenate([word, word + types[1] - types[0]], 0)
    ids = np.asarray(input_ids) + np.asarray(segment_ids) * word.shape[0]
    pooled, hidden = bert_oracle.bert_tower(sd2, prefix, ids, input_mask, n_layers, n_heads, eps, return_hidden=True)
    return hidden[-1], pooled


def brute_span(start_logits, end_logits, para_offset, length, max_answer_len=10):
    """The reader's span choice over one sequence's (fp16) logits, every (i, j) pair enumerated: score
    fp32(start[i]) + fp32(end[j]) over para_offset <= i <= j < length - 1, j - i <= max_answer_len; the highest score,
    the lowest start among equal ones, then the lowest end.  (-1, -1, -inf) without a paragraph token."""
    s = np.asarray(start_logits, np.float32)
    e = np.asarray(end_logits, np.float32)
    best, bi, bj = np.float32(-np.inf), -1, -1
    for i in range(max(para_offset, 0), length - 1):
        for j in range(i, min(i + max_answer_len, length - 2) + 1):
            v = np.float32(s[i] + e[j])
            if v > best:
                best, bi, bj = v, i, j
    return bi, bj, best
