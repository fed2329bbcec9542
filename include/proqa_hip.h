/*
 * proqa_hip.h — C ABI of libproqa_hip.so, the MI355X (gfx950) implementation of
 * ProQA's dense-retrieval hot path: corpus/query encode -> .npy index -> exhaustive
 * inner-product top-k search.
 *
 * The reference (xwhan/ProQA, pure Python) has no FFI of its own: its hot path calls
 * third-party libraries (faiss-cpu, transformers/torch).  Every entry point below
 * names the reference call site (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, a negative PROQA_E* code on failure;
 *     proqa_last_error() gives a thread-local message for the last failure.
 *   - plain pointers and sizes only; no torch / numpy types.  Pointers named *_dev are
 *     device (HBM) addresses valid on the current HIP device; all others are host.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 *   - the caller allocates every output; the library never frees caller memory.
 *   - handles are not re-entrant: one host thread per handle at a time.
 *   - one process drives one GPU (the current HIP device at handle creation).
 *   - the library has no DT_NEEDED entries for the HIP runtime and rocBLAS (the encoder's dense layers):
 *     the host process loads the pair it already uses with RTLD_GLOBAL before dlopen'ing this library
 *     (INTEGRATION.md section 3), so that device pointers and streams belong to one runtime.
 */
#ifndef PROQA_HIP_H
#define PROQA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* proqa_inbatch_eval_f16 was added WITHOUT a bump: it is purely additive (no existing symbol, struct or meaning changed),
 * and a caller that needs it finds out by looking the symbol up. */
#define PROQA_ABI_VERSION 7

/* element types of embedding matrices (the .npy index is '<f2' under --fp16, else '<f4':
 * retrieval/get_embed.py:139) */
#define PROQA_F16 0
#define PROQA_F32 1

/* error codes */
#define PROQA_OK 0
#define PROQA_EINVAL (-1)   /* bad argument */
#define PROQA_EHIP (-2)     /* HIP runtime error (message carries hipGetErrorString) */
#define PROQA_ENOMEM (-3)   /* allocation failed */
#define PROQA_EIO (-4)      /* file error */
#define PROQA_EFORMAT (-5)  /* malformed .npy */
#define PROQA_ENOGPU (-6)   /* no usable gfx950 device */

/* embedding width is hard-coded to 128 at every consumer in the reference
 * (retrieval/retriever.py:19-20, retrieval/eval_retrieval.py:98) */
#define PROQA_EMBED_DIM 128

const char* proqa_last_error(void);
int proqa_abi_version(void);
/* number of visible HIP devices, and the gcnArchName of the current one (e.g. "gfx950:...") */
int proqa_device_info(int* n_devices, char* arch_name, size_t arch_name_len);

/* ------------------------------------------------------------------------------------
 * Exact inner-product index.  Replaces
 *     index = faiss.IndexFlatIP(d); index.add(xb); D, I = index.search(xq, k)
 * at retrieval/eval_retrieval.py:102-104 (also retrieval/trec_process.py:74-76).
 * Results: scores descending; exact ties ordered by ascending row index (FAISS leaves the
 * tie order unspecified); if fewer than k rows exist the tail is I = -1, D = -FLT_MAX.
 * Scores that are not finite follow faiss's result heap: +inf ranks first; NaN and -inf never compare greater than what
 * the heap holds and are never returned (their slots count as missing rows: I = -1, D = -FLT_MAX at the tail).
 * Rows are stored in HBM as fp16 (the --fp16 index format); scores accumulate in fp32.  float32 data
 * that fp16 cannot hold is searched exactly (see proqa_index_add).
 * ---------------------------------------------------------------------------------- */
typedef struct proqa_index proqa_index;

/* d must be 128.  capacity_rows > 0 preallocates HBM for that many rows (avoids regrowth). */
int proqa_index_create(int d, int64_t capacity_rows, proqa_index** out);
/* append n rows from host memory (row-major [n, d], dtype PROQA_F16 or PROQA_F32).  May be called
 * repeatedly, e.g. once per mmap chunk of para_embed.npy.
 *
 * Precision.  The scan runs on fp16 rows.  float32 input that is exactly representable in fp16 (the
 * float32 upcast of an '<f2' index, retrieval/eval_retrieval.py:99-100) is simply stored as fp16.
 * The first float32 value fp16 cannot hold -- in an added row or in a query -- switches the index to
 * EXACT-FLOAT32 mode: it keeps a float32 copy of every row next to the fp16 roundings; the fp16 scan
 * then only nominates rows (its thresholds are lowered by a rigorous bound on the rounding error,
 * ||q^||.max||x-x^|| + ||q-q^||.max||x^|| + ...), and every nominated row is re-scored from the float32
 * data (double accumulation, rounded once).  Results are the exact float32 top-k; the scan costs the
 * same, the merge more.  Values beyond the fp16 range (|x| > 65504) are refused.
 * proqa_index_allow_rounding(idx, 1) opts out: float32 inputs are rounded to fp16 instead. */
int proqa_index_add(proqa_index* idx, const void* xb, int64_t n, int dtype);
/* np.load(path) + index.add(xb[row0:row0+n]) (retrieval/eval_retrieval.py:99-102) in one call: appends rows
 * [row0, row0 + n) of a 2-D .npy file ('<f2' or '<f4', 128 columns; n < 0 = up to the last row).  n_readers host
 * threads (<= 0: 4) pread() the rows into a ring of four pinned 8 MiB pieces while the pieces read before them travel to
 * HBM, so that the file read, the PCIe transfer and (float32 files) the conversion overlap and no pageable copy of the
 * corpus is made.  A rank of a row-sharded index loads only its own row range this way.  Same precision rules as
 * proqa_index_add.  All or nothing: on failure the index still holds the rows it had. */
int proqa_index_add_npy(proqa_index* idx, const char* path, int64_t row0, int64_t n, int n_readers);
/* same, source already in HBM (used by the synthetic benchmark and the sharded path) */
int proqa_index_add_device(proqa_index* idx, const void* xb_dev, int64_t n, int dtype, void* stream);
/* adopt caller-owned fp16 rows already in HBM without copying; the caller keeps them alive
 * until proqa_index_free/reset.  IMMUTABILITY: searches of k <= 128 over >= 65536 rows scan an int8 copy of the rows
 * (+128 B per row of HBM, see proqa_index_configure_nomination) that the library builds once and keys on the row set; a
 * caller that overwrites adopted rows in place calls proqa_index_rows_changed afterwards (or switches the copy off with
 * proqa_index_configure_nomination(idx, 0)) -- otherwise rows whose new score qualifies are searched against the stale
 * copy and can be missing from the result, silently. */
int proqa_index_adopt_device(proqa_index* idx, const void* xb_dev_f16, int64_t n);
/* the rows of the index were modified in place (adopted memory): whatever the library derived from them (the int8 copy
 * and its statistics) is rebuilt before it is used again.  Not available once the index has switched to exact-float32
 * mode (its float32 copies are the data: reset and add again). */
int proqa_index_rows_changed(proqa_index* idx);
/* Build now what the first search would otherwise build: the int8 copy of the rows for the nomination scan (an
 * allocation of 128 B per row, two passes over the rows, one host read).  Synchronises `stream`.  Optional: a
 * proqa_index_search / _search_device call builds the copy itself when it is missing or stale; an ENQUEUED search
 * (proqa_index_search_begin_device) never allocates or waits -- without a current copy it scans the fp16 rows and its
 * _finish builds the copy -- so a caller that wants its first enqueued search on the int8 copy calls this after add /
 * adopt / rows_changed.  No-op for indexes the nomination scan does not apply to. */
int proqa_index_prepare(proqa_index* idx, void* stream);
/* 1 once the index has switched to exact-float32 mode (see above) */
int proqa_index_is_exact_f32(const proqa_index* idx, int* enabled);
int proqa_index_allow_rounding(proqa_index* idx, int allow);
int proqa_index_ntotal(const proqa_index* idx, int64_t* n);
int proqa_index_reset(proqa_index* idx);
int proqa_index_free(proqa_index* idx);

/* host-pointer search: xq row-major [nq, d]; D float32 [nq, k]; I int64 [nq, k] */
int proqa_index_search(proqa_index* idx, const void* xq, int64_t nq, int dtype, int k,
                       float* D, int64_t* I);
/* device-pointer search; row indices are reported as idx_offset + local row so that a
 * row-sharded corpus yields global ids.  Synchronises `stream` before returning. */
int proqa_index_search_device(proqa_index* idx, const void* xq_dev, int64_t nq, int dtype, int k,
                              int64_t idx_offset, float* D_dev, int64_t* I_dev, void* stream);

/* Two-step form of proqa_index_search_device for a caller that has more work to put on the stream behind the search
 * (the sharded search enqueues its all-gather and merge there).  _begin enqueues the whole search and returns WITHOUT
 * synchronising or allocating whenever it can (k <= 1024 outside the one-pass range, float16 queries or float32 queries
 * of an index already in exact-float32 mode, a workspace that fits -- i.e. not the first search of its size on the
 * handle; other searches run to completion inside _begin).  It never builds the int8 copy of the rows: when that copy is
 * missing or stale the search scans the fp16 rows (same result) and _finish builds the copy after its host wait
 * (proqa_index_prepare builds it ahead of time).  Once the stream reaches that point D_dev / I_dev hold the result, provided no round overflowed its candidate
 * lists (a data-dependent, rare event): status_dev (optional device word, written on the stream) is then 0; 1 means
 * _finish is going to rewrite D_dev / I_dev.  _finish synchronises the stream, runs the overflow-safe re-scan if it is
 * needed (*rewritten = 1; D_dev / I_dev are final when it returns) and completes proqa_index_last_stats.  xq_dev, D_dev,
 * I_dev and status_dev stay valid, and no other call is made on the handle, until _finish has returned.
 * Reference call site: the one faiss search of retrieval/eval_retrieval.py:102-104 (faiss has no asynchronous form). */
int proqa_index_search_begin_device(proqa_index* idx, const void* xq_dev, int64_t nq, int dtype, int k, int64_t idx_offset,
                                    float* D_dev, int64_t* I_dev, uint32_t* status_dev, void* stream);
int proqa_index_search_finish(proqa_index* idx, int* rewritten);

/* rows of the index by id, device pointers (faiss reconstruct_batch; the gather `para_embed[I]` of
 * /root/reference/qa/online_sampler.py:117,277 without leaving the GPU): out_dev [n, d] of out_dtype.  PROQA_F16 gives
 * the stored fp16 rows; PROQA_F32 the float32 copies of an exact-float32 index, else exact upcasts of the fp16 rows --
 * in both cases the values add() was given, unless rounding was allowed.  ids are idx_offset + local row as reported
 * by the search; ids outside the index (the -1 of a short result) give zero rows.  Asynchronous on `stream`. */
int proqa_index_reconstruct_batch_device(proqa_index* idx, const int64_t* ids_dev, int64_t n, int64_t idx_offset,
                                         void* out_dev, int out_dtype, void* stream);

/* the collect step of the reference's online sampler (qa/online_sampler.py:117-136: I to the host, a dict
 * lookup and an `in gold_paras` test per id, para_embed[I] gathered and copied back) as one launch on device pointers.
 * With live(j) = idx_offset <= ids[j] < idx_offset + ntotal:
 *   rows_out[j]   = what proqa_index_reconstruct_batch_device writes for ids[j] ([k, d] of out_dtype; zero row if !live(j))
 *   labels_out[j] = 1 if live(j) and ids[j] occurs in gold_dev, else 0 (int32 [k]); gold_dev: n_gold int64 ids, strictly
 *                   ascending, in the id space of ids_dev (may be NULL when n_gold == 0)
 *   record_dev    = int64 [2 + head]: the number of live ids, the sum of labels_out, then ids[0..head) with -1 past k
 * head is in [0, 64].  k == 0 writes the record only.  The two counts are integer sums, so every output is the same bits
 * from run to run.  Asynchronous on `stream`; record_dev is written on it from its first word on. */
int proqa_sampler_collect_device(proqa_index* idx, const int64_t* ids_dev, int64_t k, int64_t idx_offset, const int64_t* gold_dev,
                                 int64_t n_gold, int head, void* rows_out_dev, int out_dtype, int32_t* labels_out_dev,
                                 int64_t* record_dev, void* stream);

/* proqa_sampler_collect_device for the n_questions result rows of one proqa_index_search_device call, in one launch per
 * 64 questions: ids_dev is int64 [n_questions, k] and, for every question q,
 *   rows_out [q], labels_out [q], record_dev [q]  ([n_questions, k, d], [n_questions, k] int32, [n_questions, 2 + head] int64)
 * hold exactly what the single entry writes for ids_dev[q] and the gold list gold_dev[gold_begin[q] .. gold_begin[q] +
 * gold_count[q]).  gold_dev is one buffer of n_gold int64 ids (the lists of all questions; strictly ascending within a
 * list; NULL when n_gold == 0); gold_begin and gold_count are HOST arrays of n_questions entries.  They are checked here
 * (a list that leaves the buffer is PROQA_EINVAL, before anything is launched) and reach the kernel by value in its
 * arguments: the call copies nothing in either direction.  Lists may be empty, may overlap and may repeat.  head is in
 * [0, 64]; k == 0 writes the records only; n_questions == 0 does nothing.  Integer sums only: the same bits from run to
 * run.  Asynchronous on `stream`; the library zeroes the counts of every record on it, so record_dev is written on the
 * stream from its first word on and needs no preparation.  Added WITHOUT a bump of PROQA_ABI_VERSION (purely additive). */
int proqa_sampler_collect_multi_device(proqa_index* idx, const int64_t* ids_dev, int64_t n_questions, int64_t k, int64_t idx_offset,
                                       const int64_t* gold_dev, int64_t n_gold, const int64_t* gold_begin, const int64_t* gold_count,
                                       int head, void* rows_out_dev, int out_dtype, int32_t* labels_out_dev, int64_t* record_dev,
                                       void* stream);

/* statistics of the last search on this handle (for tests and the benchmark) */
typedef struct proqa_search_stats {
  int32_t rounds;            /* filter+merge rounds launched */
  int32_t fallback_rounds;   /* rounds run again: slabs re-scanned on the overflow-safe path, and the rounds of the second
                                search that the queries a leaping round left short are given (proqa_index_configure_leap) */
  int64_t candidates;        /* (score,id) pairs that passed the running threshold */
  float filter_ms;           /* HIP-event time of the mips_filter launches, summed over the
                                rounds (0 unless profiling is enabled on the handle) */
  float total_ms;            /* HIP-event time of the whole search on the stream */
  int64_t nominated;         /* rows the int8 nomination rounds handed to the exact re-scoring (0 for an fp16 scan) */
  int32_t nomination;        /* 1 if the rounds of this search scanned the int8 copy of the rows, else 0 */
  int32_t nomination_state;  /* of the index after this search: 0 off (mode 0 / exact-float32), 1 on (the copy is, or will
                                be, scanned by the searches it applies to), 2 suspended (the rows do not quantise, or a
                                search over-nominated: fp16 scan until a re-probe succeeds or the rows change) */
  int32_t leap_rank;         /* > 0: the rounds of this search tested against the score at that rank (< k) of the running lists
                                (leaping rounds, proqa_index_configure_leap); 0: against the k-th best, as ever */
  int32_t leap_state;        /* of the index after this search: 0 off (mode 0 / exact-float32), 1 on, 2 paused (leaping
                                rounds fell short: ordinary rounds for the next 16, 32, ... 1024 eligible searches) */
} proqa_search_stats;
int proqa_index_last_stats(const proqa_index* idx, proqa_search_stats* out);
/* bracket every mips_filter launch with HIP events on the search stream (bench.py roofline) */
int proqa_index_set_profiling(proqa_index* idx, int enable);
/* tuning knobs of the round schedule (0 keeps the default): rows of the first slab (scanned with
 * threshold -inf) and the growth factor of the following slabs */
int proqa_index_configure(proqa_index* idx, int first_slab_rows, int growth);
/* rows whose exact top-k a search takes from a dense score matrix (two launches) before the threshold rounds start;
 * a multiple of 32 up to 8192, 0 disables it.  Used for k <= rows/4 (at most 256) on indexes of >= 4*rows rows;
 * the result never depends on it.  Default 4096. */
int proqa_index_configure_bootstrap(proqa_index* idx, int rows);
/* The int8 nomination scan of the k <= 128 rounds (fp16 indexes of >= 65536 rows): the
 * rounds scan an int8 copy of the centred, per-dimension-scaled rows at twice the fp16 MFMA rate, nominate every row whose
 * integer score exceeds the running threshold lowered by a rigorous bound on the quantisation error, and re-score the
 * nominated rows from the fp16 rows -- the result is the fp16 scan's, bit for bit.  mode 0: never (fp16 scan);
 * 1 (default, automatic): a search that re-scores more than max(4096, rows / 2048) rows per query or needs the
 * overflow-safe path SUSPENDS the int8 rounds (fp16 scan); the 8th eligible search after that probes them again, a
 * failed probe doubles the distance (16, 32, 64, 64, ...), a successful one resumes; a change of the rows starts afresh;
 * every switch is one line on stderr when PROQA_LOG is set, and proqa_search_stats.nomination_state reports the state;
 * 2: always.  A search with k in the thousands for a FEW queries (one question, k = 5000: rows >= 16 x queries x ~1.5 k) scans
 * the copy as well, in its one launch over the shard (same result; mode 0 keeps the fp16 rows).  The copy (+128 B per row) is
 * built by proqa_index_prepare, or by the first search that wants it.  Rows
 * adopted with proqa_index_adopt_device: see the immutability note there. */
int proqa_index_configure_nomination(proqa_index* idx, int mode);
/* Leaping rounds of the k <= 128 searches (fp16 indexes, default schedule, behind the bootstrap).  A round that tests against
 * the k-th best score of the n0 rows seen so far logs ~k (rho - 1) candidates per query while the rows seen grow by rho --
 * which is what keeps rho near 3 and an 18M-row search at eight rounds.  A LEAPING round tests against the score at rank
 * j < k of the running list: it logs ~j (rho - 1) rows, so rho can be 5-16 and the rounds three or four.  Its result is exact
 * iff at least k rows of everything seen so far beat that threshold (every one of them is then known); the round's merge
 * checks exactly that, and a round that falls short is re-scanned against the k-th best scores on the overflow-safe path
 * (proqa_search_stats.fallback_rounds) -- the result never depends on the leap.  j is the smallest rank for which the
 * shortfall has probability <= 1e-8 per query and round when the first rows stand for the rest (rows in no particular
 * order: the count of new rows above the rank-j score is negative-binomial (j, 1 / rho)).  What a shortfall costs: the
 * queries that fell short are searched again as a batch of their own on ordinary rounds and their result rows rewritten
 * (every other query's result is verified): ~ +10 % of the search for a handful, at most one more search for all of them
 * (the flagged slabs are re-scanned for all queries only when a list or a merge overflowed as well).  Rows sorted by topic
 * or norm -- or long runs of near-duplicates: ~k/2 rows that score alike next to each other -- make leaps fall short:
 * up to 256 short queries count three strikes (a clean leap takes one back), more eight; at eight strikes the leaps of the
 * index pause for 16
 * eligible searches, a failed retry doubles the pause (up to 1024), a clean one clears it, changed rows start afresh; one
 * stderr line per event under PROQA_LOG.  mode 0: never; 1 (default): automatic, as above.  An index configured with
 * proqa_index_configure(growth) keeps its ordinary rounds. */
int proqa_index_configure_leap(proqa_index* idx, int mode);
/* The schedule proqa_index_configure_leap's automatic mode takes for a search of `queries` queries for the best k of `rows`
 * rows behind a bootstrap of `bootstrap_rows` (host arithmetic only, no GPU): rounds behind the bootstrap (0: no leap --
 * k > 128 or k < 8, or nothing fits the merges), the rank j < k its thresholds sit at, the rows expected above a threshold
 * per round and query (j (rho - 1), rho = (rows / bootstrap_rows)^(1 / rounds)) and the probability that fewer than k - j rows
 * beat it -- the negative-binomial (j, 1 / rho) sum -- per query and round.  nominating: the rounds scan the int8 copy (their
 * merges hold 2048 nominated rows).  rows_per_round / shortfall_probability may be NULL. */
int proqa_leap_plan(int64_t rows, int64_t bootstrap_rows, int k, int64_t queries, int nominating, int* rounds, int* rank,
                    double* rows_per_round, double* shortfall_probability);

/* Merge n_parts per-shard result lists into one: D_parts/I_parts are [n_parts, nq, k]
 * (the layout an RCCL all-gather of per-rank [nq, k] produces); every list as a search reports it (scores descending,
 * ties by ascending id, the I = -1 slots of a short shard at its tail), parts in ascending order of their row ranges.
 * Same ordering rule.  These two entry points SORT what they are given (no assumption about the order inside a part: a
 * caller's own local search may have produced it): up to 16384 gathered keys per query in LDS, larger merges (k = 10000 x
 * 8 shards) as a segmented radix sort in HBM (temporary buffers are allocated for the call).  The sharded search's own
 * merge (proqa_topk_merge_gathered_device, below) knows its parts are search results and merges up to 4096 keys per query
 * (8 shards x top-80) by rank, without a sort. */
int proqa_topk_merge_device(const float* D_parts_dev, const int64_t* I_parts_dev, int n_parts,
                            int64_t nq, int k, float* D_dev, int64_t* I_dev, void* stream);
/* The same merge over parts that are not back to back: part p's [nq, k] scores / ids start stride_d / stride_i ELEMENTS
 * after part p-1's -- the receive buffer of ONE all-gather whose per-rank block holds the ids followed by the scores
 * is merged where it lies (D_parts = buffer + ids bytes, stride_d = block bytes / 4, stride_i = block bytes / 8). */
int proqa_topk_merge_strided_device(const float* D_parts_dev, const int64_t* I_parts_dev, int n_parts, int64_t nq, int k,
                                    int64_t stride_d, int64_t stride_i, float* D_dev, int64_t* I_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Encoder: BertForRetriever.get_embed (retrieval/retriever.py:33-43 + transformers BertModel)
 * as one call: embeddings -> n_layers x {QKV, attention, output dense + LN, FFN + LN} ->
 * pooler (tanh dense on h[:,0]) -> Linear(hidden, 128).
 * All weights are device pointers to fp16, dense weights row-major [out, in] (the layout of the
 * reference checkpoint, cast to fp16); qkv_w / qkv_b are the query|key|value weights stacked
 * along `out` ([3*hidden, hidden] / [3*hidden]).  The caller owns the weights and keeps them
 * alive while the encoder exists.  The dense layers are rocBLAS GEMMs (fp32 accumulate).
 * ------------------------------------------------------------------------------------ */
typedef struct proqa_bert_layer {
  const void *qkv_w, *qkv_b;      /* [3*hidden, hidden], [3*hidden] */
  const void *ao_w, *ao_b;        /* attention.output.dense */
  const void *ln1_g, *ln1_b;      /* attention.output.LayerNorm */
  const void *ff1_w, *ff1_b;      /* intermediate.dense  [intermediate, hidden] */
  const void *ff2_w, *ff2_b;      /* output.dense        [hidden, intermediate] */
  const void *ln2_g, *ln2_b;      /* output.LayerNorm */
} proqa_bert_layer;

typedef struct proqa_bert_weights {
  int32_t hidden, n_layers, n_heads, intermediate, max_position;
  int64_t vocab;
  float layer_norm_eps;
  const void *word_emb, *pos_emb, *type_emb;   /* type_emb: row 0 (token_type_ids are never passed) */
  const void *emb_ln_g, *emb_ln_b;
  const proqa_bert_layer* layers;              /* n_layers entries (copied by create) */
  const void *pool_w, *pool_b;                 /* pooler.dense */
  const void *proj_w, *proj_b;                 /* proj_q / proj_c: [128, hidden], [128]; both NULL for a tower without a
                                                  projection (the reader's bert: proqa_encoder_forward_hidden only) */
} proqa_bert_weights;

typedef struct proqa_encoder proqa_encoder;

#define PROQA_ENC_CLS_ONLY_LAST 1  /* last layer: attention output / dense blocks / LayerNorms for the [CLS] rows only */
#define PROQA_ENC_PACKED 2         /* evaluate the valid tokens only (needs n_valid_tokens) */

int proqa_encoder_create(const proqa_bert_weights* w, proqa_encoder** out);
int proqa_encoder_free(proqa_encoder* enc);
/* opt-in (off by default): the first forward that meets a large GEMM shape times every rocBLAS solution for
 * it on the real operands (~0.3 s per shape) and keeps the winner if an interleaved re-match confirms >= 2 %;
 * same arithmetic (fp16 in, fp32 accumulate), possibly another summation order. */
int proqa_encoder_set_gemm_tuning(proqa_encoder* enc, int enable);
/* Which library kernel runs the large dense layers (QKV, attention output, FFN2; FFN1 is proqa_gemm_tn_f16).  hipBLASLt's
 * own choice for these shapes is 3-20 % slower than the best kernel it holds, so the encoder calls hipBLASLt itself with an
 * algorithm chosen BY KERNEL NAME from a fixed preference list (csrc/lt_gemm.cpp) -- deterministic, no timing at run time;
 * with a library build that does not know the names, or without hipBLASLt in the process, the layers run on
 * rocblas_gemm_ex.  name_out receives the pinned kernel's name ("" = rocblas_gemm_ex: no name matched, or no large product
 * has run yet on this handle), truncated to name_len - 1 characters. */
int proqa_encoder_gemm_kernel(const proqa_encoder* enc, char* name_out, size_t name_len);
/* The activation workspace of the handle: base address and size (0 / 0 before the first forward).  A forward over more
 * tokens or sequences than any before it REPLACES the workspace; a caller that captured forwards of this handle into a HIP
 * graph (proqa_amd.online_retriever.GraphedQuestionEncoder) compares the base address before a replay and re-captures when
 * it has changed.  forward itself is capturable once the workspace fits: no allocation, no host synchronisation. */
int proqa_encoder_workspace(const proqa_encoder* enc, void** base_out, size_t* bytes_out);
/* The library dense layer of this handle on its own (tests): out[m, n] = x[m, k] . w[n, k]^T, fp16 row-major device
 * pointers, fp32 accumulate -- the pinned hipBLASLt kernel where it applies, else rocblas_gemm_ex (small_dense_mfma for
 * <= 256 rows).  Asynchronous on `stream`. */
int proqa_encoder_dense(proqa_encoder* enc, const void* x_dev, const void* w_dev, void* out_dev, int64_t m, int n, int k,
                        void* stream);
/* ids_dev: [batch, seq_len] int64, right-padded (retrieval/datasets.py:29-45); seq_lens_dev: [batch]
 * int32 valid lengths (>= 1); n_valid_tokens: their sum if the host knows it, else -1 (then the
 * padded layout is evaluated whatever the flags say); out: [batch, 128] of out_dtype.
 * Asynchronous on `stream`; not re-entrant per handle. */
int proqa_encoder_forward(proqa_encoder* enc, const int64_t* ids_dev, const int32_t* seq_lens_dev, int batch,
                          int seq_len, int64_t n_valid_tokens, int flags, void* out, int out_dtype, void* stream);

/* The tower up to its last hidden state, with token-type (segment) embeddings: BertModel(input_ids, input_mask,
 * token_type_ids) of the reader (qa/bert_retrieve_qa.py:58-62).  Every layer runs for every token (no [CLS]-only last
 * layer); no projection.
 *   type_ids_dev:   int64 laid out like ids_dev, or NULL = all 0 (then the table below may be NULL: weights' type_emb row 0)
 *   type_emb_table: the full [n_types, hidden] fp16 token_type_embeddings table (ids outside [0, n_types) read row 0)
 *   Layout is the caller's choice: flags = PROQA_ENC_PACKED (n_valid_tokens = sum of the lengths, required) writes
 *   hidden_out packed [n_valid_tokens, hidden] (sequence b from row cu_seqlens[b], the exclusive prefix sum of seq_lens);
 *   flags = 0 writes [batch * seq_len, hidden] (padding rows hold finite values nothing should read).  No other flag.
 *   pooled_out: [batch, hidden] fp16 tanh pooler output (BertModel(...)[1]), or NULL.
 * Same workspace and capture rules as proqa_encoder_forward; works on a handle created with or without a projection. */
int proqa_encoder_forward_hidden(proqa_encoder* enc, const int64_t* ids_dev, const int64_t* type_ids_dev,
                                 const void* type_emb_table, int n_types, const int32_t* seq_lens_dev, int batch,
                                 int seq_len, int64_t n_valid_tokens, int flags, void* hidden_out, void* pooled_out,
                                 void* stream);

/* ------------------------------------------------------------------------------------
 * Reader head (qa/bert_retrieve_qa.py:58-77 + the span choice of qa/train_retrieve_qa.py:300-313) over the hidden
 * states of proqa_encoder_forward_hidden, one launch for a batch of [CLS] q [SEP] p [SEP] sequences:
 *   logit[t] = fp16(fp32(hidden[t] . qa_w[k]) + qa_b[k]), k = 0 start / 1 end  (a half-precision nn.Linear(hidden, 2))
 *   span of sequence b = argmax over para_offset[b] <= i <= j < len(b) - 1, j - i <= max_answer_len, of
 *     score = fp32(start[i]) + fp32(end[j])   (the paragraph mask: [para_offset, len - 1))
 *   TIE RULE: the lowest start, then the lowest end (the reference's CPU argmax: row maxima first, then that row's end).
 *   A sequence without a paragraph token gets start = end = -1, score = -inf (the reference raises IndexError there).
 *   A start whose candidate scores are all -inf or NaN (fp16 logits that overflowed) is skipped; if every start is, the
 *   sequence reports no span the same way, where the reference would still return some span.
 * Layout: exactly one of seq_lens_dev (padded: sequence b is rows b * seq_len .., len(b) = seq_lens[b]) and cu_seqlens_dev
 * (packed: rows cu_seqlens[b] .. cu_seqlens[b + 1], [batch + 1] int32) is non-NULL; seq_len is the padded row stride,
 * or in the packed layout any bound on the longest sequence (<= 4096).  para_offset_dev [batch] int32.
 * Outputs (device): start_out / end_out [batch] int32 positions within the sequence, score_out [batch] fp32, logits_out
 * (optional) [rows, 2] fp16 (start, end) for the valid rows.  hidden and qa_w 16-byte aligned; hidden <= 1024. */
int proqa_reader_span_f16(const void* hidden, const int32_t* seq_lens_dev, const int32_t* cu_seqlens_dev, int batch,
                          int seq_len, int hidden_size, const int32_t* para_offset_dev, const void* qa_w, const void* qa_b,
                          int max_answer_len, int32_t* start_out, int32_t* end_out, float* score_out, void* logits_out,
                          void* stream);
/* proqa_reader_span_f16 with the first n_best spans of every sequence and the log-partitions of its logits, in the same
 * single launch (hidden is read once, no [L, L] tensor).  Added WITHOUT a bump of PROQA_ABI_VERSION (purely additive).
 *   Layouts, logits (same device function, same bits), paragraph mask and candidates are those of proqa_reader_span_f16: a
 *   candidate is (i, j), para_offset[b] <= i <= j < len(b) - 1, j - i <= max_answer_len, score = fp32(start[i]) +
 *   fp32(end[j]), and a score that is -inf or NaN is no candidate (+inf is one).
 *   ORDER: score descending (-0 equals +0), then start ascending, then end ascending -- a total order, so the result does not
 *   depend on scheduling.  Row b of start_out / end_out / score_out [batch, n_best] holds the first n_best candidates in that
 *   order and (-1, -1, -inf) where there are fewer; entry 0 equals proqa_reader_span_f16's output in all three fields, bit
 *   for bit.  score_out holds the fp32 sum itself.
 *   lse_out [batch, 2] fp32 = (Z^s_b, Z^e_b): the log-sum-exp of the fp16 start / end logits over the paragraph rows
 *   [para_offset[b], len(b) - 1) of sequence b alone -- what proqa_reader_loss_f16 keeps in stats without the shared norm,
 *   not bit for bit: here max + log(sum exp(x - max)) with every sum in a fixed order (no atomics, bit-identical from run to
 *   run).  -inf for an empty paragraph or one whose logits are all -inf; +inf when a logit is +inf; NaN when one is NaN.
 *   P(span | sequence) = exp(score - Z^s - Z^e) under a per-passage norm; the shared norm of training is the host's
 *   log-sum-exp of these over a question's sequences (proqa_amd.qa_utils.marginal_answers).
 * Limits: 1 <= n_best <= 32, max_answer_len >= 0, otherwise those of proqa_reader_span_f16; anything else is PROQA_EINVAL
 * before the device is touched.  logits_out optional, as there. */
int proqa_reader_span_nbest_f16(const void* hidden, const int32_t* seq_lens_dev, const int32_t* cu_seqlens_dev, int batch,
                                int seq_len, int hidden_size, const int32_t* para_offset_dev, const void* qa_w,
                                const void* qa_b, int max_answer_len, int n_best, int32_t* start_out, int32_t* end_out,
                                float* score_out, float* lse_out, void* logits_out, void* stream);
/* select_outputs = Linear(hidden, 1) on the pooled output (--add-select): out[b] = fp16(pooled[b] . select_w + select_b),
 * returned as fp32 [batch] (device).  pooled [batch, hidden] and select_w [hidden] fp16, 16-byte aligned. */
int proqa_reader_select_f16(const void* pooled, int batch, int hidden_size, const void* select_w, const void* select_b,
                            float* out, void* stream);

/* The kernels the encoder is made of, individually (tests, other drivers). */
/* y[m,n] = epilogue(x[m,k] . w[n,k]^T + bias[n]): the encoder's dense layer as a hand-written MFMA GEMM (fp16 in, fp32
 * accumulate, fp16 out; 256 x 256 x 64 tiles, LDS-DMA ring).  epilogue 0: none (bias ignored), 1: + bias,
 * 2: erf-GELU(. + bias) = BertIntermediate.  m and n multiples of 256, k a multiple of 64; x, w, y and a non-NULL bias
 * 16-byte aligned (rows are dense: x [m, k], w [n, k], y [m, n]); anything else is PROQA_EINVAL before any launch, m = 0
 * is PROQA_OK and writes nothing.  The contract as tests/test_gemm_gpu.py holds it, element by element against float64:
 *   - the sum is accumulated in fp32 (fp16 subnormal operands count in full) and rounded once to fp16 after the epilogue; a
 *     result beyond fp16's range is the correctly rounded +-Inf (after the GELU a pre-activation below -65504 gives 0);
 *   - the GELU is max(t, 0) - a Phi(-a), a = min(|t|, 6), with Phi(-a) = 2^q(a), q a degree-6 fit: off by at most
 *     4.6e-5 a Phi(-a) from the erf form before rounding (relative to Phi(-a): the negative tail keeps its accuracy), and
 *     its fp16 result is the correctly rounded one or its neighbour (one step off for ~2 % of all fp16 arguments).  It is
 *     built on max(): a NaN pre-activation comes out of epilogue 2 as a finite number (-6 Phi(-6), i.e. -0), and -Inf as 0;
 *     epilogues 0 and 1 hand NaN and Inf on.  An operand's Inf / NaN reaches its own output row / column only;
 *   - results do not depend on the base alignment, are bit-identical from launch to launch, and nothing outside y is written;
 *   - the launch is min(tiles, max(CU count, 8)) persistent workgroups: the tile walk assigns the 256-row slabs by
 *     blockIdx.x & 7 and needs all 8 residues whenever there are more slabs than workgroups. */
#define PROQA_GEMM_EPI_NONE 0
#define PROQA_GEMM_EPI_BIAS 1
#define PROQA_GEMM_EPI_BIAS_GELU 2
int proqa_gemm_tn_f16(const void* x_dev, const void* w_dev, const void* bias_dev, void* y_dev, int64_t m, int n, int k,
                      int epilogue, void* stream);
/* out[b,s,:] = LayerNorm(word[ids[b,s]] + pos[s] + type[0]) , eps = 1e-12
 * (BertEmbeddings; token_type_ids are never passed by the reference => row 0) */
int proqa_embed_layernorm_f16(const int64_t* ids_dev, int64_t n_tokens, int seq_len, int hidden,
                              const void* word_emb, int64_t vocab, const void* pos_emb,
                              const void* type_emb, const void* ln_gamma, const void* ln_beta,
                              float eps, void* out, void* stream);

/* the same with token types: out[t] = LayerNorm(word[ids[t]] + pos[t % seq_len] + type_table[type_ids[t]]), type_ids int64
 * laid out like ids (NULL = all 0; ids outside [0, n_types) read row 0); BertEmbeddings with token_type_ids */
int proqa_embed_layernorm_typed_f16(const int64_t* ids_dev, const int64_t* type_ids_dev, int64_t n_tokens, int seq_len,
                                    int hidden, const void* word_emb, int64_t vocab, const void* pos_emb,
                                    const void* type_emb_table, int n_types, const void* ln_gamma, const void* ln_beta,
                                    float eps, void* out, void* stream);

/* Packed ("varlen") token layout: sequences are stored back to back without padding rows,
 * cu_seqlens[b] = first row of sequence b, cu_seqlens[batch] = total tokens (int32, device).
 * Every per-token operator is unchanged on the packed [T, hidden] matrix; only the embedding
 * gather and the attention need the offsets.  Results for the valid tokens equal the padded
 * evaluation (padding never reaches a valid token: retrieval/datasets.py:29-45 pads on the right,
 * the attention masks those keys).
 * ids stay padded [batch, seq_len] (as em_collate produces them); out_packed is [T, hidden]. */
int proqa_embed_layernorm_varlen_f16(const int64_t* ids_dev, const int32_t* cu_seqlens_dev, int batch,
                                     int seq_len, int hidden, const void* word_emb, int64_t vocab,
                                     const void* pos_emb, const void* type_emb, const void* ln_gamma,
                                     const void* ln_beta, float eps, void* out_packed, void* stream);
/* packed layout with token types (type_ids padded [batch, seq_len] like ids, NULL = all 0) */
int proqa_embed_layernorm_typed_varlen_f16(const int64_t* ids_dev, const int64_t* type_ids_dev,
                                           const int32_t* cu_seqlens_dev, int batch, int seq_len, int hidden,
                                           const void* word_emb, int64_t vocab, const void* pos_emb,
                                           const void* type_emb_table, int n_types, const void* ln_gamma,
                                           const void* ln_beta, float eps, void* out_packed, void* stream);

/* fused multi-head self-attention for one layer:
 *   ctx = softmax(Q K^T / sqrt(64) + key_mask) V,   head_dim 64
 * qkv is the fused projection output [B*S, 3*hidden] (Q | K | V, each head-major);
 * seq_lens[b] = number of valid (unpadded) keys of sequence b — the reference pads on the
 * right with mask False (retrieval/datasets.py:29-45,298-305). */
int proqa_attention_f16(const void* qkv, const int32_t* seq_lens_dev, int batch, int seq_len,
                        int n_heads, void* ctx_out, void* stream);

/* the same attention for query row 0 ([CLS]) of every sequence only: ctx_cls_out [B, hidden].
 * Only h[:, 0] of the last layer reaches the pooler (retrieval/retriever.py:41-42), so the last
 * layer's attention output / FFN are computed for that row alone. */
int proqa_attention_cls_f16(const void* qkv, const int32_t* seq_lens_dev, int batch, int seq_len,
                            int n_heads, void* ctx_cls_out, void* stream);

/* the two attention entry points on the packed layout: qkv_packed [T, 3*hidden], ctx_packed_out
 * [T, hidden] (ctx_cls_out stays [batch, hidden]); max_seq_len = longest sequence of the batch */
int proqa_attention_varlen_f16(const void* qkv_packed, const int32_t* cu_seqlens_dev, int batch,
                               int max_seq_len, int n_heads, void* ctx_packed_out, void* stream);
int proqa_attention_cls_varlen_f16(const void* qkv_packed, const int32_t* cu_seqlens_dev, int batch,
                                   int max_seq_len, int n_heads, void* ctx_cls_out, void* stream);
/* general form of the four entry points above, with the bias of the fused Q|K|V projection folded in
 * (qkv_bias [3*hidden] fp16 or NULL): the query bias is added to the query fragments, the key bias is
 * dropped (it shifts all scores of a query by the same amount: softmax-invariant), the value bias is
 * added to the output (probabilities sum to 1).  Exactly one of seq_lens_dev (padded layout) and
 * cu_seqlens_dev (packed layout) is non-NULL; cls_only selects the [batch, hidden] row-0 output.
 * That is the full kernel (cls_only = 0).  The cls_only kernel adds all three biases to the rows it reads: it works on
 * q + b_q, k + b_k and v + b_v, each rounded to fp16 as a half-precision dense layer would have stored them.  Same
 * mathematics, other roundings: a large key bias costs its keys the bits below the bias' own fp16 spacing.
 * Lengths are clamped to [1, seq_len].
 * Padded layout: the K and V of the rows >= len are never read.  The outputs of the valid queries do not depend on what
 * those rows hold, bit for bit, NaN and Inf included.  The output rows >= len are written (their queries are the padding
 * rows' own Q) and hold values nothing should read. */
int proqa_attention_ex_f16(const void* qkv, const void* qkv_bias, const int32_t* seq_lens_dev,
                           const int32_t* cu_seqlens_dev, int batch, int seq_len, int n_heads, int cls_only,
                           void* out, void* stream);

/* x = gelu_erf(x + bias) in place, x [rows, cols] (BertIntermediate, hidden_act='gelu') */
int proqa_bias_gelu_f16(void* x, const void* bias, int64_t rows, int cols, void* stream);

/* out = LayerNorm(x + bias + residual) (BertSelfOutput / BertOutput), eps = 1e-12 */
int proqa_bias_residual_layernorm_f16(const void* x, const void* bias, const void* residual,
                                      const void* gamma, const void* beta, float eps,
                                      int64_t rows, int cols, void* out, void* stream);

/* embed[b,:] = (tanh(h[b,0,:] Wp^T + bp)) Wproj^T + bproj
 * (BertPooler + proj_{q,c}: retrieval/retriever.py:19-20,37-42).  h is [B, S, hidden];
 * pooled_ws is caller-provided scratch of B*hidden fp16; out is [B, 128] in out_dtype. */
int proqa_pool_project_f16(const void* h, int batch, int seq_len, int hidden, const void* w_pool,
                           const void* b_pool, const void* w_proj, const void* b_proj,
                           void* pooled_ws, void* out, int out_dtype, void* stream);

/* The dense layer for a few token rows on its own (what proqa_encoder_dense and the encoder's FFN run for <= 256 rows):
 *   y[rows, n_feat] = act(x[rows, k] . w[n_feat, k]^T + bias[n_feat]),  act 0: none, 1: erf-GELU (BertIntermediate)
 * fp16 row-major device pointers, fp32 accumulate; bias [n_feat] fp16 or NULL.  Any rows >= 0 (the grid grows with it);
 * n_feat a multiple of 32 and k a multiple of 128, anything else is PROQA_EINVAL before the device is touched.
 * Added WITHOUT a bump of PROQA_ABI_VERSION (purely additive). */
int proqa_small_dense_f16(const void* x, int rows, const void* w, const void* bias, int n_feat, int k, int act, void* y,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * Backward operators of the tower and of the in-batch objective: what `loss.backward()` of retriever pre-training
 * (retrieval/train_retriever.py:196-214) runs between the dense products.  Added WITHOUT a bump of PROQA_ABI_VERSION
 * (purely additive).  Common rules: fp16 device operands in the packed token layout, every sum in fp32; a gradient of an
 * fp16 activation is written as fp16, a parameter-vector or embedding-table gradient as fp32; every operator is linear in
 * its incoming gradient and passes inf / NaN through (no data-dependent loop); no allocation, no host synchronisation;
 * everything on `stream`.  The forward operators save nothing: each backward recomputes what it needs from the forward's
 * own inputs.  Apart from d_word, every output is bit-identical from run to run (d_word too through the *_det entry points).
 * ws / ws_bytes: caller-owned device scratch of at least proqa_backward_workspace_bytes(cols) bytes (the attention:
 * proqa_attention_backward_workspace_bytes), 16-byte aligned; contents undefined afterwards; calls that share a
 * workspace must be ordered on one stream.
 * ---------------------------------------------------------------------------------- */
size_t proqa_backward_workspace_bytes(int cols);
size_t proqa_attention_backward_workspace_bytes(int64_t n_tokens, int n_heads);
/* out[c] = sum_r x[r, c]: x [rows, cols] fp16 -> out [cols] fp32, rows added in a fixed order (slabs of rows, then the slabs
 * in ascending order).  The bias gradient of a dense layer whose bias a fused operator did not own (the Q|K|V bias:
 * column sum of d_qkv).  cols a multiple of 8, <= 8192. */
int proqa_colsum_f16(const void* x, int64_t rows, int cols, float* out, void* ws, size_t ws_bytes, void* stream);
/* out = gelu_erf(x + bias), out of place (proqa_bias_gelu_f16 overwrites the operand its backward needs) */
int proqa_bias_gelu_out_f16(const void* x, const void* bias, int64_t rows, int cols, void* out, void* stream);
/* dx = dy * gelu'(x_pre + bias), gelu'(t) = Phi(t) + t phi(t) (the derivative of the erf form); dbias [cols] fp32 = column
 * sum of dx before its rounding.  cols a multiple of 8, <= 8192. */
int proqa_bias_gelu_backward_f16(const void* dy, const void* x_pre, const void* bias, int64_t rows, int cols, void* dx,
                                 float* dbias, void* ws, size_t ws_bytes, void* stream);
/* backward of out = LayerNorm(x + bias + residual) * gamma + beta: dz [rows, cols] fp16 is the gradient of x and of
 * residual alike; dgamma, dbeta, dbias [cols] fp32 (dbias = column sum of dz before its rounding).  Mean and variance
 * are recomputed from x + bias + residual in fp32.  cols a multiple of 8, <= 1024. */
int proqa_bias_residual_layernorm_backward_f16(const void* dy, const void* x, const void* bias, const void* residual,
                                               const void* gamma, float eps, int64_t rows, int cols, void* dz, float* dgamma,
                                               float* dbeta, float* dbias, void* ws, size_t ws_bytes, void* stream);
/* backward of proqa_embed_layernorm_varlen_f16: dy [n_tokens, hidden] packed, ids padded [batch, seq_len] (ids at or past a
 * sequence's length contribute nothing), seq_len <= 512.  All five outputs are fp32 and ADDED INTO buffers the caller
 * zeroed: dgamma, dbeta, d_type0 [hidden], d_pos [>= seq_len, hidden] (rows past the longest sequence stay untouched),
 * d_word [vocab, hidden] (fp32 atomics: the one output whose bits depend on the order of execution). */
int proqa_embed_layernorm_varlen_backward_f16(const void* dy, const int64_t* ids_dev, const int32_t* cu_seqlens_dev,
                                              int batch, int seq_len, int hidden, int64_t n_tokens, const void* word_emb,
                                              int64_t vocab, const void* pos_emb, const void* type_emb, const void* ln_gamma,
                                              float eps, float* dgamma, float* dbeta, float* d_word, float* d_pos,
                                              float* d_type0, void* ws, size_t ws_bytes, void* stream);
/* backward of proqa_embed_layernorm_typed_varlen_f16 (the reader's [CLS] q [SEP] p [SEP] with segment ids); the rules and
 * the arguments of proqa_embed_layernorm_varlen_backward_f16, with: type_ids_dev int64 padded [batch, seq_len] like ids
 * (NULL: every token has type 0); type_emb_table [n_types, hidden] fp16; d_types [n_types, hidden] fp32, ADDED INTO like
 * the other four.  n_types must be 1 or 2 (BERT's type_vocab_size).  A type id outside [0, n_types) read row 0 in the
 * forward and its gradient goes to row 0; likewise a word id outside the vocabulary.  Everything but d_word is
 * bit-identical from run to run: a workgroup owns a position, keeps its sum in two parts (tokens of type 0, of type 1),
 * d_pos[s] is their sum and d_types[t] the sum over the positions of part t, in ascending order.  With type_ids NULL,
 * dgamma / dbeta / d_pos / d_types[0] carry the bits of the untyped entry point.  ws: at least
 * proqa_embed_layernorm_typed_backward_workspace_bytes(hidden) bytes (four quantities per position, one more than
 * proqa_backward_workspace_bytes provides).  PROQA_EINVAL before any launch for n_types, hidden % 8, hidden > 1024,
 * seq_len > 512, a short workspace or a NULL argument other than type_ids_dev. */
size_t proqa_embed_layernorm_typed_backward_workspace_bytes(int hidden);
int proqa_embed_layernorm_typed_varlen_backward_f16(const void* dy, const int64_t* ids_dev, const int64_t* type_ids_dev,
                                                    const int32_t* cu_seqlens_dev, int batch, int seq_len, int hidden,
                                                    int64_t n_tokens, const void* word_emb, int64_t vocab,
                                                    const void* pos_emb, const void* type_emb_table, int n_types,
                                                    const void* ln_gamma, float eps, float* dgamma, float* dbeta,
                                                    float* d_word, float* d_pos, float* d_types, void* ws, size_t ws_bytes,
                                                    void* stream);
/* The two embedding backwards with d_word summed in a FIXED ORDER: every output is then bit-identical from run to run.  The
 * arguments, the ADDED-INTO rule and the refusals are those of the entry points above; dgamma, dbeta, d_pos and d_type0 /
 * d_types carry the bits of those entry points.  d_word, so that a caller can predict its bits:
 *   - the occurrences of a word id k are the tokens whose clamped id is k (an id outside [0, vocab) counts as 0; ids at or
 *     past a sequence's length are never read), taken in ascending packed row cu_seqlens[b] + s: n_k of them;
 *   - dz_t is the fp32 per-token gradient that the atomic entry points add (the same arithmetic, hence the same bits);
 *   - the occurrences are cut into chunks of C = proqa_embed_word_grad_chunk(), counted from the id's first occurrence;
 *   - a chunk's partial is the sequential fp32 sum ((dz_0 + dz_1) + dz_2) + ..., each add rounded to nearest;
 *   - the id's sum is the sequential fp32 sum of its chunk partials in ascending order;
 *   - d_word[k] = d_word[k] + that sum, one add; rows of ids that do not occur are neither read nor written.
 * The association depends on n_k alone: not on the grid, on timing or on the other ids of the batch.  No float atomics;
 * a device-side radix sort of (id, row) finds the occurrences; no allocation, no host synchronisation, no workgroup waits
 * on another.  Linear in dy; inf / NaN reach the rows of their tokens' ids and no others.
 * ws: at least proqa_embed_layernorm_backward_det_workspace_bytes(n_tokens, hidden, typed) bytes (typed = 1 for the typed
 * entry point), which covers the atomic entry point's need and the sort's; non-decreasing in n_tokens.  PROQA_EINVAL
 * before any launch for everything the entry points above refuse, for a short workspace, and for vocab or n_tokens of
 * 2^31 - 1 or more (the sort's key holds each in 32 bits). */
int proqa_embed_word_grad_chunk(void);
size_t proqa_embed_layernorm_backward_det_workspace_bytes(int64_t n_tokens, int hidden, int typed);
int proqa_embed_layernorm_varlen_backward_det_f16(const void* dy, const int64_t* ids_dev, const int32_t* cu_seqlens_dev,
                                                  int batch, int seq_len, int hidden, int64_t n_tokens, const void* word_emb,
                                                  int64_t vocab, const void* pos_emb, const void* type_emb,
                                                  const void* ln_gamma, float eps, float* dgamma, float* dbeta, float* d_word,
                                                  float* d_pos, float* d_type0, void* ws, size_t ws_bytes, void* stream);
int proqa_embed_layernorm_typed_varlen_backward_det_f16(const void* dy, const int64_t* ids_dev, const int64_t* type_ids_dev,
                                                        const int32_t* cu_seqlens_dev, int batch, int seq_len, int hidden,
                                                        int64_t n_tokens, const void* word_emb, int64_t vocab,
                                                        const void* pos_emb, const void* type_emb_table, int n_types,
                                                        const void* ln_gamma, float eps, float* dgamma, float* dbeta,
                                                        float* d_word, float* d_pos, float* d_types, void* ws,
                                                        size_t ws_bytes, void* stream);
/* backward of proqa_attention_ex_f16 on the packed layout (cls_only = 0): qkv [n_tokens, 3*hidden] (the GEMM output before
 * the bias), qkv_bias [3*hidden] or NULL, d_ctx [n_tokens, hidden] -> d_qkv [n_tokens, 3*hidden], every element written.
 * The probabilities are recomputed with the forward's conventions (query bias added, key bias dropped, scores / 8, fp32
 * statistics); all five products run on v_mfma_f32_32x32x16_f16.  The gradient of qkv_bias is the column sum of d_qkv
 * (proqa_colsum_f16); its key third is zero up to rounding.  max_seq_len <= 512, head_dim 64; n_tokens =
 * cu_seqlens[batch]; a sequence whose offsets fall outside [0, n_tokens] is skipped. */
int proqa_attention_backward_f16(const void* qkv, const void* qkv_bias, const void* d_ctx, const int32_t* cu_seqlens_dev,
                                 int batch, int max_seq_len, int n_heads, int64_t n_tokens, void* d_qkv, void* ws,
                                 size_t ws_bytes, void* stream);
/* ------------------------------------------------------------------------------------
 * Dropout of the towers in training (transformers' hidden_dropout_prob and attention_probs_dropout_prob), inside the fused
 * operators.  Added WITHOUT a bump of PROQA_ABI_VERSION (purely additive); the rules of the backward block above hold.
 * A mask is never stored: it is a pure function of (seed, site, call, coordinates) -- Philox4x32-10 with key
 * (seed & 0xffffffff, seed >> 32), csrc/dropout_rng.h -- and every kernel regenerates the bits it needs, the backward
 * kernels the same bits as the forward.  An element is kept iff its 16 bits >= thr = min(65535, floor(p * 65536 + 0.5));
 * the effective rate is thr / 65536 and the survivors are multiplied by 1 / (1 - thr / 65536) (fp32).  p in [0, 1).
 * site in [0, 255]: 0 the embeddings, 1 + 3 * layer + {0: attention probabilities, 1: attention output, 2: FFN output};
 * call: the caller's count of tower passes, 24 bits (it wraps).
 *   hidden element (row, col) of a [rows, cols] matrix: counter (col >> 3, row, 0, site | call << 8),
 *                                                       word (col & 7) >> 1, half col & 1;  rows < 2^32
 *   probability (b, head, query i, key j):              counter (j >> 2, i >> 1, b * n_heads + head, site | call << 8),
 *                                                       word j & 3, half i & 1
 * ---------------------------------------------------------------------------------- */
#define PROQA_DROPOUT_HIDDEN 0
#define PROQA_DROPOUT_PROBS 1
/* Pure host function, no GPU needed: keep[t] = 1 if the element is kept, else 0, for n consecutive values c0 .. c0 + n - 1
 * of the last coordinate.  PROQA_DROPOUT_HIDDEN: a = row, b ignored, c = column.  PROQA_DROPOUT_PROBS: a = b * n_heads +
 * head, b = query, c = key. */
int proqa_dropout_keep_host(int kind, double p, uint64_t seed, int site, uint32_t call, int64_t a, int64_t b, int64_t c0,
                            int64_t n, uint8_t* keep);
/* out = x * keep * factor on [rows, cols] fp16 (the product in fp32, rounded once; a dropped element is +0).  The
 * embeddings: transformers drops after the embedding LayerNorm.  Its backward is the same call on dy.  cols % 8 == 0. */
int proqa_dropout_f16(const void* x, int64_t rows, int cols, double p, uint64_t seed, int site, uint32_t call, void* out,
                      void* stream);
/* out = LayerNorm(dropout(x + bias) + residual) * gamma + beta: transformers' order, the dense bias inside the dropout.
 * Otherwise proqa_bias_residual_layernorm_f16. */
int proqa_bias_residual_layernorm_dropout_f16(const void* x, const void* bias, const void* residual, const void* gamma,
                                              const void* beta, float eps, int64_t rows, int cols, double p, uint64_t seed,
                                              int site, uint32_t call, void* out, void* stream);
/* its backward: dresidual [rows, cols] fp16 = dz, dx = dz * keep * factor, dbias = the fp32 column sum of dx before its
 * rounding; dgamma, dbeta and every rule as proqa_bias_residual_layernorm_backward_f16. */
int proqa_bias_residual_layernorm_dropout_backward_f16(const void* dy, const void* x, const void* bias, const void* residual,
                                                       const void* gamma, float eps, int64_t rows, int cols, double p,
                                                       uint64_t seed, int site, uint32_t call, void* dx, void* dresidual,
                                                       float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes,
                                                       void* stream);
/* proqa_attention_ex_f16 on the packed layout with dropout of the probabilities: ctx = (P D)(V + b_v), D = factor where
 * kept and 0 elsewhere.  The softmax statistics run over all keys; dropped probabilities are zero in the fp16 operand of
 * P V and the factor enters once, with 1 / l.  The rows of P D do not sum to 1: the value bias is weighted by
 * factor * l_kept / l (l_kept = the fp32 sum of the kept probabilities).  The key bias is still dropped. */
int proqa_attention_dropout_f16(const void* qkv, const void* qkv_bias, const int32_t* cu_seqlens_dev, int batch,
                                int max_seq_len, int n_heads, double p, uint64_t seed, int site, uint32_t call, void* ctx_out,
                                void* stream);
/* its backward, as proqa_attention_backward_f16 (same workspace): dV = (P D)^T dO, dP = D (dO (V + b_v)^T) -- the value
 * bias does not drop out of dP here --, delta = sum_k P dP, dS = P (dP - delta).  The gradient of qkv_bias is still the
 * column sum of d_qkv. */
int proqa_attention_dropout_backward_f16(const void* qkv, const void* qkv_bias, const void* d_ctx,
                                         const int32_t* cu_seqlens_dev, int batch, int max_seq_len, int n_heads,
                                         int64_t n_tokens, double p, uint64_t seed, int site, uint32_t call, void* d_qkv,
                                         void* ws, size_t ws_bytes, void* stream);
/* gradient of loss = mean_i (lse_i - s[i, target_i]), s = q c^T (CrossEntropyLoss(q @ c.T, target),
 * retrieval/train_retriever.py:203-205): q [nq, 128], c [nc, 128], target as proqa_inbatch_eval_f16 (NULL = the diagonal;
 * several questions may share a target; a target outside [0, nc) has no gold term), lse [nq] fp32 as that call produced
 * it, grad_in: device pointer to the fp32 scalar incoming gradient.  dq [nq, 128], dc [nc, 128] fp16.  The score matrix
 * exists one 32 x 32 tile at a time. */
int proqa_inbatch_loss_grad_f16(const void* q, const void* c, const int32_t* target, const float* lse, const float* grad_in,
                                int nq, int nc, int dim, void* dq, void* dc, void* stream);
/* ------------------------------------------------------------------------------------
 * The block-diagonal in-batch objective: M micro-batches of one accumulation window in one call (pretrain_retriever.py
 * --micro-batches-per-pass).  Added WITHOUT a bump of PROQA_ABI_VERSION (purely additive).
 * q, c [n, 128] fp16 (device, 16-byte aligned); block_offsets: HOST int32 [n_blocks + 1], ascending from 0 to n, read
 * during the call and handed to the kernels by value.  Block m owns the rows [o_m, o_{m+1}) of BOTH q and c: row i of the
 * block has its gold at column i and its log-sum-exp runs over the block's columns only, as if
 * proqa_inbatch_eval_f16(q + o_m, c + o_m, NULL, n_m, n_m, ...) had been called per block.
 *   lse_out, gold_out  fp32 [n]
 *   loss_out           fp32 [n_blocks]: mean_i (lse_i - gold_i) over the block's rows, summed in a fixed order
 * The gradient call takes lse as the first call wrote it and grad_in, DEVICE fp32 [n_blocks], one incoming gradient per
 * block: d s[i, j] = grad_in[m] / n_m (exp(s[i, j] - lse_i) - [i == j]) inside block m.  Nothing outside a block is read
 * for it and nothing outside it contributes: a non-finite row or grad_in[m] reaches block m only.  dq, dc [n, 128] fp16.
 * Bit rule: the block launches run the kernel bodies of proqa_inbatch_eval_f16 / proqa_inbatch_loss_grad_f16 with the
 * block on a grid dimension and the row pointers offset (a row is 256 bytes: every slice stays 16-byte aligned); no
 * workgroup or wave holds rows of two blocks, and the block launch never splits a block's columns.  The single eval call
 * makes no column split when ceil(n_m / 32) <= 16, i.e. n_m <= 512 (a split is no finer than 4 column tiles for each of
 * the 4 waves: at most ceil(tiles / 16) splits).  For every block with n_m <= 512, lse,
 * gold, dq and dc therefore carry the BITS of the single calls on the block's slices; a larger block differs from the
 * single call in the order of its log-sum-exp merges only.  n_blocks == 1 forms every index the single calls form.
 * Limits: 1 <= n_blocks <= PROQA_INBATCH_MAX_BLOCKS, every block at least one row, n <= 2^24, dim == 128; anything else
 * is PROQA_EINVAL before the device is touched.  No allocation, no host synchronisation, no atomics: bit-identical from
 * run to run.
 * ---------------------------------------------------------------------------------- */
#define PROQA_INBATCH_MAX_BLOCKS 64
int proqa_inbatch_loss_blocks_f16(const void* q, const void* c, const int32_t* block_offsets, int n_blocks, int n, int dim,
                                  float* lse_out, float* gold_out, float* loss_out, void* stream);
int proqa_inbatch_loss_blocks_grad_f16(const void* q, const void* c, const int32_t* block_offsets, int n_blocks, int n, int dim,
                                       const float* lse, const float* grad_in, void* dq, void* dc, void* stream);
/* ------------------------------------------------------------------------------------
 * The reader's training objective (qa/bert_retrieve_qa.py:64-171 with --shared-norm, joint loss and early loss, as
 * qa/train_dense_qa.sh trains it) on the hidden states of B sequences [CLS] q [SEP] p [SEP] of ONE question, and its
 * gradient.  Added WITHOUT a bump of PROQA_ABI_VERSION (purely additive); the rules of the backward block above hold:
 * every sum in fp32, linear in the incoming gradient, inf / NaN pass through, no allocation, no host synchronisation, no
 * atomics, bit-identical from run to run.
 *   s_b[t], e_b[t]   the logits of proqa_reader_span_f16 (same device function, same bits): fp16(fp32(hidden[t] . qa_w[k]) +
 *                    qa_b[k]); rows outside the paragraph mask [para_offset[b], len(b) - 1) count as -inf.  With p > 0 the
 *                    hidden row is dropped first: PROQA_DROPOUT_HIDDEN at (packed row, column) -- the packed row in both
 *                    layouts --, factor applied in fp32; site 255 is reserved for this head.
 *   Z^s, Z^e         fp32 log-sum-exp of s / e over the paragraph rows: of all sequences with
 *                    PROQA_READER_LOSS_SHARED_NORM, of each sequence on its own without
 *   r                softmax_j(q . para_embed[j]) over all n_paras rows, the dot products in fp32; the first `batch` rows
 *                    belong to the sequences, in order.  Z^r = their log-sum-exp
 *   l_ba             s_b[start_pos[b, a]] - Z^s + e_b[end_pos[b, a]] - Z^e + log r_b for a pair whose two positions lie inside
 *                    the sequence's paragraph mask (positions are sequence coordinates, -1 = padding); other pairs count as 0
 *   joint            -logsumexp over the valid pairs of l_ba, or 0 when no pair is valid
 *   early            -(logsumexp over labels[j] != 0 of log r_j), or 0 when no label is set or PROQA_READER_LOSS_NO_EARLY
 *   loss_out[3]      = (joint + early, joint, early), fp32
 * Layout of hidden / logits as proqa_reader_span_f16: exactly one of seq_lens_dev (padded) and cu_seqlens_dev (packed).
 * start_pos / end_pos: int32 [batch, n_answers].  q: fp16 [128].  para_embed: [n_paras, 128] of para_dtype (PROQA_F16 or
 * PROQA_F32), labels int32 [n_paras].  logits_out: fp16 [rows, 2], the unmasked logits of every valid row (the padded
 * layout's padding rows are zeros).
 * stats: fp32 [8 + 2 * batch], what the backward needs of the forward: [0] joint, [1] Z^r, [2] the log-sum-exp of the gold
 * rows' scores, [3] 1 if a pair is valid else 0, [4] 1 if the early term is live else 0, [5..7] 0, then (Z^s_b, Z^e_b) of
 * every sequence (the same pair for all under the shared norm).
 * Limits: hidden_size % 8 == 0 and <= 1024, dim == 128, 1 <= batch <= n_paras <= 65536, 1 <= n_answers <= 1024,
 * seq_len <= 4096; anything else is PROQA_EINVAL before the device is touched.  hidden, qa_w, q, para_embed, ws 16-byte
 * aligned.  ws / ws_bytes: caller-owned scratch of at least proqa_reader_loss_workspace_bytes(...) bytes (a pure host
 * function; 0 for sizes out of range); contents undefined afterwards, the backward reads nothing the forward left there. */
#define PROQA_READER_LOSS_SHARED_NORM 1
#define PROQA_READER_LOSS_NO_EARLY 2
size_t proqa_reader_loss_workspace_bytes(int batch, int seq_len, int hidden_size, int n_answers, int n_paras);
int proqa_reader_loss_f16(const void* hidden, const int32_t* seq_lens_dev, const int32_t* cu_seqlens_dev, int batch,
                          int seq_len, int hidden_size, const int32_t* para_offset_dev, const void* qa_w, const void* qa_b,
                          const int32_t* start_pos, const int32_t* end_pos, int n_answers, const void* q,
                          const void* para_embed, int para_dtype, const int32_t* labels, int n_paras, int dim, int flags,
                          double p, uint64_t seed, int site, uint32_t call, void* logits_out, float* stats, float* loss_out,
                          void* ws, size_t ws_bytes, void* stream);
/* Its gradient, times the fp32 device scalar *grad_in.  With w_ba = exp(l_ba + joint), omega_b = sum_a w_ba and W^s_b[t] /
 * W^e_b[t] the sums of the w_ba whose start / end is t:
 *   dlogit        ds_b[t] = c_b exp(s_b[t] - Z^s) - W^s_b[t] (c_b = 1 under the shared norm, omega_b without), likewise de;
 *                 zero outside the mask and when no pair is valid.  It exists in fp32 registers only.
 *   d_hidden      fp16, laid out like hidden: (ds w_0 + de w_1) * keep * factor in fp32, rounded once.  EVERY element is
 *                 written: rows outside the mask and the padded layout's padding rows are zeros.
 *   d_qa_w [2, hidden_size], d_qa_b [2]   fp32: sum_t dlogit[t, k] * (dropped) hidden[t] and sum_t dlogit[t, k]; workgroup
 *                 slabs added in ascending order.
 *   d_q [128]     fp16: sum_j drank_j para_embed[j], drank_j = (r_j - omega_j [j < batch]) + (r_j - g_j), g_j = r_j / (sum of
 *                 the gold r) on gold rows; each bracket is dropped with the loss term it belongs to.
 * logits and stats as the forward wrote them for the same operands. */
int proqa_reader_loss_backward_f16(const void* hidden, const int32_t* seq_lens_dev, const int32_t* cu_seqlens_dev, int batch,
                                   int seq_len, int hidden_size, const int32_t* para_offset_dev, const void* qa_w,
                                   const int32_t* start_pos, const int32_t* end_pos, int n_answers, const void* q,
                                   const void* para_embed, int para_dtype, const int32_t* labels, int n_paras, int dim,
                                   int flags, double p, uint64_t seed, int site, uint32_t call, const void* logits,
                                   const float* stats, const float* grad_in, void* d_hidden, float* d_qa_w, float* d_qa_b,
                                   void* d_q, void* ws, size_t ws_bytes, void* stream);
/* The same objective over n_questions questions in ONE call (three launches forward, four backward, whatever n_questions
 * is): the same seven kernels with a question dimension; the single-question entry points above are their one-question
 * case.  Added WITHOUT a bump of PROQA_ABI_VERSION (purely additive); every rule of the block above holds.
 * Packed layout only: hidden [T, hidden_size] with cu_seqlens_dev [batch + 1] over the sequences of ALL questions,
 * para_offset_dev [batch], start_pos / end_pos [batch, n_answers]; para_embed [n_paras, 128] / labels [n_paras] hold the
 * questions' rows one question after the other; q fp16 [n_questions, 128]; one qa_w / qa_b / flags / para_dtype / dropout
 * tuple for the call.  Device CSR arrays, int32 [n_questions + 1]: question i owns the sequences question_seq_dev[i] ..
 * question_seq_dev[i + 1] (B_i of them) and the rows question_para_dev[i] .. question_para_dev[i + 1] of para_embed / labels
 * (P_i of them, the first B_i belong to its sequences, in order).  max_seqs / max_paras: the largest B_i / P_i; with
 * n_questions, batch and seq_len they size the grids, nothing is read back.
 * Outputs: loss_out fp32 [n_questions, 3] = (total, joint, early) per question; logits_out [T, 2]; stats fp32
 * [8 * n_questions + 2 * batch]: the single-question layout question after question (question i's block starts at
 * 8 * i + 2 * question_seq[i]).  Backward: grad_in fp32 [n_questions], one incoming gradient per question; d_hidden
 * [T, hidden_size], d_q fp16 [n_questions, 128], ONE d_qa_w [2, hidden_size] / d_qa_b [2].
 * CONTRACT: loss_out[i], the logits of question i's rows, its block of stats, its rows of d_hidden and d_q[i] carry the
 * bits the single-question entry points return for the question's slice of the operands -- rows cu[first sequence] ..
 * cu[last sequence + 1] of hidden, cu_seqlens rebased to 0, its rows of para_embed / labels, q[i], grad_in[i] -- with p == 0.
 * d_qa_w / d_qa_b: question i's value is the compensated ascending slab sum the single call makes for the slice at the SAME
 * seq_len (seq_len fixes the slabs per sequence, and the compensated sum is taken over all of them); the values are added
 * in ascending question order by plain fp32 additions, starting from question 0's value: ((v_0 + v_1) + v_2) + ...
 * With p > 0 the mask coordinate is the packed row of the WHOLE pack (site 255, one `call` for the pass), so the masks of
 * different questions are independent; this is the one place where a slice call (whose rows count from 0) differs.
 * Limits, PROQA_EINVAL before the device is touched: 1 <= n_questions <= 4096; n_questions <= batch <= 65536;
 * batch <= n_paras <= 4194304 (2^22); max_seqs / max_paras possible maxima of n_questions counts >= 1 that sum to batch /
 * n_paras, max_seqs <= max_paras <= 65536; hidden_size, n_answers, seq_len, dim and the alignments as the single call.
 * question_seq_host / question_para_host: host copies of the two arrays, both or neither.  Given, every question is checked
 * as well (the arrays run from 0 to batch / n_paras, 1 <= B_i <= P_i, B_i <= max_seqs, P_i <= max_paras).  The DEVICE
 * arrays cannot be checked without a read-back: the kernels clamp every entry into [0, batch] / [0, n_paras] and make each
 * pair ascending, and take at most max_paras rows per question, so arrays that are not ascending or do not cover batch /
 * n_paras give wrong values (a question left with no sequence, or fewer rows than sequences, gets a zero loss and no
 * gradient) and never an access out of range.
 * ws: at least proqa_reader_loss_multi_workspace_bytes(...) bytes (a pure host function; 0 for sizes out of range). */
size_t proqa_reader_loss_multi_workspace_bytes(int n_questions, int batch, int seq_len, int hidden_size, int n_answers,
                                               int n_paras, int max_paras);
int proqa_reader_loss_multi_f16(const void* hidden, const int32_t* cu_seqlens_dev, int batch, int seq_len, int hidden_size,
                                const int32_t* para_offset_dev, const void* qa_w, const void* qa_b, const int32_t* start_pos,
                                const int32_t* end_pos, int n_answers, const void* q, const void* para_embed, int para_dtype,
                                const int32_t* labels, int n_paras, int dim, const int32_t* question_seq_dev,
                                const int32_t* question_para_dev, int n_questions, int max_seqs, int max_paras,
                                const int32_t* question_seq_host, const int32_t* question_para_host, int flags, double p,
                                uint64_t seed, int site, uint32_t call, void* logits_out, float* stats, float* loss_out,
                                void* ws, size_t ws_bytes, void* stream);
int proqa_reader_loss_multi_backward_f16(const void* hidden, const int32_t* cu_seqlens_dev, int batch, int seq_len,
                                         int hidden_size, const int32_t* para_offset_dev, const void* qa_w,
                                         const int32_t* start_pos, const int32_t* end_pos, int n_answers, const void* q,
                                         const void* para_embed, int para_dtype, const int32_t* labels, int n_paras, int dim,
                                         const int32_t* question_seq_dev, const int32_t* question_para_dev, int n_questions,
                                         int max_seqs, int max_paras, const int32_t* question_seq_host,
                                         const int32_t* question_para_host, int flags, double p, uint64_t seed, int site,
                                         uint32_t call, const void* logits, const float* stats, const float* grad_in,
                                         void* d_hidden, float* d_qa_w, float* d_qa_b, void* d_q, void* ws, size_t ws_bytes,
                                         void* stream);
/* The weight gradient of a linear layer y = x w^T, on a kernel of our own (csrc/linear_kernels.hip) so that it never
 * passes through fp16: fp16 operands, ONE fp32 sum over the whole token axis on v_mfma_f32_32x32x16_f16, fp32 output
 * written or accumulated straight into the caller's buffer.  Added WITHOUT a bump of PROQA_ABI_VERSION (purely additive).
 * dw[N, K] (fp32, row-major, contiguous) = (accumulate ? dw : 0) + sum_t dy[t, n] * x[t, k]
 * dy [T, N], x [T, K]: fp16, row-major, contiguous, 16-byte aligned (dw and ws too).  T >= 0, N % 8 == 0, K % 8 == 0.
 * T == 0 writes zeros, or leaves dw alone when accumulate is set.  The token axis is cut into `splits` slices
 * (proqa_linear_wgrad_plan with the device's compute-unit count); with splits > 1 the partial tiles go through ws
 * (at least the plan's ws_bytes; contents undefined afterwards, nothing of its previous contents is read) and are added
 * in ascending slice order, the existing dw last.  No atomics: bit-identical from run to run.  Rows of dw whose dy column
 * holds an inf / NaN come out non-finite, every other row is untouched by it (likewise columns and x). */
int proqa_linear_wgrad_f16(const void* dy, const void* x, int64_t T, int N, int K, float* dw, int accumulate,
                           void* ws, size_t ws_bytes, void* stream);
/* Pure host function, no GPU needed: how many slices of the token axis a launch on n_cus compute units uses, and the
 * workspace it needs (0 when splits == 1, else splits * N * K * 4).  Slice boundaries are multiples of the kernel's
 * contraction step of 32 tokens; no slice is empty. */
int proqa_linear_wgrad_plan(int64_t T, int N, int K, int n_cus, int* splits, size_t* ws_bytes);

/* ------------------------------------------------------------------------------------
 * The optimizer step of retriever training: what retrieval/train_retriever.py:207-214 runs between loss.backward() and the
 * next forward (amp's unscale and overflow check, clip_grad_norm_, transformers.AdamW.step) as three launches over all
 * parameter tensors at once.  Added WITHOUT a bump of PROQA_ABI_VERSION (purely additive).  Rules of the backward block:
 * caller-owned workspace and state, no allocation, no host synchronisation, everything on `stream`.
 *
 * All tensors are contiguous fp32 in HBM, 4-byte aligned; a tensor whose p, g, m and v are all 16-byte aligned takes the
 * 16-byte path.  One workgroup owns one fixed chunk of PROQA_ADAMW_CHUNK elements of one tensor in both passes; the chunk
 * map depends on the sizes only and is built once (proqa_adamw_chunk_map).  The tensor table and the chunk map are DEVICE
 * arrays: the caller refreshes the table's g / lr / weight_decay each step with an asynchronous copy on `stream` (from
 * pinned memory it does not reuse before that copy has run), so the host never waits.
 *
 * One step (proqa_adamw_step), with s = the loss scale in the state:
 *   1. partial[c] = sum over chunk c of (g / s)^2 in fp32 (unscaled before squaring), a fixed order, no atomics;
 *   2. one workgroup adds the partials in ascending chunk order in double (256 contiguous runs, then the runs in order):
 *      norm = sqrt(sum) is what clip_grad_norm_ returns; found_inf = norm is not finite;
 *      clip = min(1, max_grad_norm / (norm + 1e-6)) (exactly 1 below the limit or without one);
 *      found_inf: skipped += 1 and (dynamic scale) s *= backoff_factor, clean_steps = 0;
 *      otherwise: step += 1, bias corrections 1 - beta^step in double, and (dynamic scale) clean_steps += 1, at
 *      growth_interval: s *= growth_factor, clean_steps = 0 (apex amp's scaler, which the reference trains with);
 *   3. found_inf: nothing is written.  Otherwise per element, fp32, g' = g * (clip / s):
 *        m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2
 *        reference (transformers.AdamW, correct_bias): p -= lr sqrt(bc2) / bc1 * m / (sqrt(v) + eps);  p -= lr wd p
 *        torch_semantics (torch.optim.AdamW):          p *= 1 - lr wd;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
 *      A tensor with g = NULL is skipped in 1 and 3 (p, m, v untouched).  ONE step count for all tensors (both originals
 *      count per parameter; they differ only for a parameter that had no gradient in some step).
 * Without clipping (max_grad_norm <= 0) and without a scale (PROQA_ADAMW_SCALE_NONE) launches 1 and 2 are skipped, the
 * state is not touched (state_dev, ws may be NULL) and the step number is the caller's host_step.
 * Results are bit-identical from run to run.
 * proqa_adamw_step_half is the same step that also writes an fp16 working copy of every tensor it updates (mixed
 * precision: the forward's weights without a cast per forward); proqa_cast_half_tensors writes the copies alone.
 * ---------------------------------------------------------------------------------- */
#define PROQA_ADAMW_CHUNK 16384
#define PROQA_ADAMW_SCALE_NONE 0      /* gradients are not scaled (the state's scale is 1) */
#define PROQA_ADAMW_SCALE_FIXED 1     /* the state's scale never changes */
#define PROQA_ADAMW_SCALE_DYNAMIC 2
typedef struct proqa_adamw_tensor {
  void* p;            /* [n] parameter */
  const void* g;      /* [n] gradient, or NULL: the tensor is skipped */
  void* m;            /* [n] exp_avg */
  void* v;            /* [n] exp_avg_sq */
  int64_t n;
  double lr;
  double weight_decay;
} proqa_adamw_tensor;
typedef struct proqa_adamw_chunk {
  int32_t tensor;     /* row of the tensor table */
  int32_t index;      /* elements [index * PROQA_ADAMW_CHUNK, ...) of that tensor */
} proqa_adamw_chunk;
typedef struct proqa_adamw_hyper {
  double beta1, beta2, eps;
  float max_grad_norm;       /* <= 0: no clipping */
  int32_t torch_semantics;
  int32_t scale_mode;        /* PROQA_ADAMW_SCALE_* */
  float backoff_factor;      /* dynamic scale: 0.5 */
  float growth_factor;       /* dynamic scale: 2 */
  int32_t growth_interval;   /* dynamic scale: 2000 */
  int64_t host_step;         /* used only when launches 1 and 2 are skipped: the number of this step, >= 1 */
} proqa_adamw_hyper;
/* Device scalars of the optimizer, PROQA_ADAMW_STATE_BYTES of caller-owned device memory (8-byte aligned), written by
 * proqa_adamw_state_init and by every step.  Byte offsets: 0 int64 step; 8 int64 skipped steps; 16 int64 clean steps;
 * 24 float loss scale; 28 float norm of the last step (unscaled, before clipping); 32 int32 found_inf of the last step;
 * 36 float gradient factor clip / scale; 40, 48 double bias corrections; 56 float clip coefficient; 60 reserved. */
#define PROQA_ADAMW_STATE_BYTES 64
/* chunks of the tensors of these sizes, in table order (host arrays; a size-0 tensor has none).  Returns the number of
 * chunks, or a negative error; out = NULL only counts, otherwise out holds `capacity` entries. */
int64_t proqa_adamw_chunk_map(const int64_t* sizes, int n_tensors, proqa_adamw_chunk* out, int64_t capacity);
size_t proqa_adamw_workspace_bytes(int64_t n_chunks);
/* (re)start the state: step counts and the loss scale (> 0, finite; 1 for PROQA_ADAMW_SCALE_NONE; apex starts a dynamic
 * scale at 65536).  One tiny launch on `stream`. */
int proqa_adamw_state_init(void* state_dev, int64_t step, float loss_scale, int64_t clean_steps, int64_t skipped_steps,
                           void* stream);
int proqa_adamw_step(const proqa_adamw_tensor* table_dev, int n_tensors, const proqa_adamw_chunk* chunks_dev, int64_t n_chunks,
                     const proqa_adamw_hyper* hyper, void* state_dev, void* ws, size_t ws_bytes, void* stream);
/* as proqa_adamw_step; half_dev: DEVICE array of n_tensors pointers (or NULL = proqa_adamw_step).  half_dev[t] != NULL:
 * every element of tensor t that launch 3 writes is also written to half_dev[t][i] as fp16, round to nearest even from
 * the fp32 value just stored in p (beyond +-65504 -> +-inf, as p.to(float16)).  Nothing else changes: p, m, v and the
 * state get the bits proqa_adamw_step gives them.  A skipped step (found_inf) and a tensor with g = NULL write no copy
 * (p did not change, so the copy is still p's).  A copy is [n] fp16, 2-byte aligned; one that is 8-byte aligned (with p,
 * g, m, v 16-byte aligned) is written with 8-byte stores, any other with 2-byte stores.  Which loop computes p, m, v is
 * decided by the alignment of p, g, m, v alone, as in proqa_adamw_step. */
int proqa_adamw_step_half(const proqa_adamw_tensor* table_dev, void* const* half_dev, int n_tensors,
                          const proqa_adamw_chunk* chunks_dev, int64_t n_chunks, const proqa_adamw_hyper* hyper, void* state_dev,
                          void* ws, size_t ws_bytes, void* stream);
/* half_dev[t][i] = (fp16) p[i] for every tensor with a copy: one launch over the same chunk map (only p and n of the
 * table are read).  For construction, after load_state_dict, after any edit of the masters that did not go through the
 * step. */
int proqa_cast_half_tensors(const proqa_adamw_tensor* table_dev, void* const* half_dev, int n_tensors,
                            const proqa_adamw_chunk* chunks_dev, int64_t n_chunks, void* stream);

/* ------------------------------------------------------------------------------------
 * Trainer-state snapshot: all fp32 tensors of a training run (masters, exp_avg, exp_avg_sq, the optimizer's device
 * scalars viewed as fp32) copied into one flat device buffer and digested, in TWO launches whatever n_tensors is.  Added
 * WITHOUT a bump of PROQA_ABI_VERSION (purely additive).  Rules of the optimizer block: caller-owned buffers, no
 * allocation, no host synchronisation, no atomics, everything on `stream`; two calls on the same memory execute the same
 * instruction stream.
 *
 * Layout.  Tensor t is numel[t] contiguous fp32 words at src_dev_ptrs[t] (a DEVICE array of n_tensors device pointers,
 * so that a table survives tensors that move); the words are copied AS BITS (NaN payloads, -0.0 and denormals keep their
 * bits) to dst_flat_dev + dst_offsets[t].  dst_flat_dev and every dst_offsets[t] (bytes) are multiples of
 * PROQA_STATE_DST_ALIGN; the bytes between one tensor's end and the next one's start are not written.
 * dst_flat_dev == NULL: digest only (dst_offsets may be NULL).  numel and dst_offsets are HOST arrays.  0 <= numel[t] <=
 * 2^31 (a larger tensor is refused with PROQA_EINVAL); numel[t] == 0 and n_tensors == 0 are valid.
 *
 * Digest.  digests_dev[t] (DEVICE, n_tensors x uint64) = sum over i in [0, numel[t]) of mix(bits_i, i) mod 2^64 with
 *     mix(bits, i) = ((uint64)(bits ^ PROQA_STATE_MIX_XOR) * (2 i + 1)) mod 2^64,
 * bits_i the 32-bit pattern of element i, i its 64-bit index inside the tensor; an empty tensor has digest 0.  For
 * i < 2^31 the weight 2 i + 1 is an odd 32-bit number that no other index has, hence: changing one element changes the
 * digest (a non-zero difference below 2^32 times a weight below 2^32 is non-zero mod 2^64), and so does swapping two
 * unequal elements ((a - b) (w_i - w_j) != 0, below 2^64 in magnitude).  The xor makes a zero-filled tensor's digest
 * depend on its length.  One workgroup owns one chunk of PROQA_STATE_CHUNK elements and writes one uint64 partial; one
 * wave per tensor then adds the tensor's partials.
 *
 * Alignment.  A source is only guaranteed 4-byte aligned (a parameter may be a row slice of a flat buffer): per chunk the
 * elements before the first 16-byte boundary and the up to three after the last are loaded as single words, everything
 * between with 16-byte loads.  A 16-byte aligned source is stored with 16-byte stores, a shifted one with 4-byte stores.
 *
 * Workspace.  ws (DEVICE, 16-byte aligned, proqa_state_snapshot_workspace_bytes) = [plan | partials].  The plan
 * (proqa_state_snapshot_plan_bytes: n_tensors x proqa_state_tensor, then one proqa_state_chunk per chunk in tensor order)
 * depends on numel and dst_offsets only: proqa_state_snapshot_plan fills a HOST image that the caller uploads to the start
 * of ws once; the calls read it and write the partials behind it.  The three size / plan functions are pure host functions
 * (no GPU needed); the size functions return 0 for sizes that proqa_state_snapshot refuses (proqa_last_error says why).
 * ---------------------------------------------------------------------------------- */
#define PROQA_STATE_CHUNK 16384
#define PROQA_STATE_DST_ALIGN 256
#define PROQA_STATE_MIX_XOR 0x9E3779B9u
typedef struct proqa_state_tensor {
  int64_t numel;
  int64_t dst_offset;    /* bytes into dst_flat_dev */
  int64_t first_chunk;   /* index of the tensor's first chunk (and partial) */
  int64_t n_chunks;      /* ceil(numel / PROQA_STATE_CHUNK) */
} proqa_state_tensor;
typedef struct proqa_state_chunk {
  int32_t tensor;
  int32_t index;         /* elements [index * PROQA_STATE_CHUNK, ...) of that tensor */
} proqa_state_chunk;
size_t proqa_state_snapshot_plan_bytes(const int64_t* numel, int n_tensors);
size_t proqa_state_snapshot_workspace_bytes(const int64_t* numel, int n_tensors);
int proqa_state_snapshot_plan(const int64_t* numel, const int64_t* dst_offsets, int n_tensors, void* plan_host,
                              size_t plan_bytes);
int proqa_state_snapshot(const void* const* src_dev_ptrs, const int64_t* numel, int n_tensors, void* dst_flat_dev,
                         const int64_t* dst_offsets, uint64_t* digests_dev, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * k-means over passage embeddings.  Replaces faiss.Clustering.train + index.search(data, 1) of
 * retrieval/group_paras.py:20-53 (IndexFlatL2, IndexFlatIP when --spherical).  The Lloyd loop
 * (sampling, initialisation, empty-cluster splitting: faiss Clustering.cpp) runs on the host
 * (proqa_amd/group_paras.py); these are its two heavy steps.  Points are fp16 [n,128] in HBM,
 * centroids float32 [k,128] in HBM (fp32-grade dot products: hi/lo split on the matrix pipe).
 * ---------------------------------------------------------------------------------- */
typedef struct proqa_kmeans proqa_kmeans;
int proqa_kmeans_create(int d, int64_t n_max, int k, proqa_kmeans** out);
int proqa_kmeans_free(proqa_kmeans* h);
/* nearest centroid of every point: assign int32 [n]; dist float32 [n] = squared L2 distance
 * (metric_l2 != 0) or inner product; exact ties go to the lowest centroid index.
 * Supported range: every centroid component a finite number of at most 65504 in size (what fp16 holds), and for the L2
 * metric |c| <= 65504 for every centroid (its -|c|^2/2 rides on the matrix pipe as five fp16 terms, exact up to there).
 * Centroids outside it are refused with PROQA_EINVAL and nothing is written to assign / dist: the centroid preparation
 * raises a word on the device, the assignment kernels queued behind it leave at once when it is set, and the call
 * returns once that word has reached the host: it waits for the work queued on `stream` BEFORE it and for the centroid
 * preparation (microseconds), not for the assignment, which is still asynchronous.  Points are any fp16 values; a point
 * with a non-finite component gets an unspecified label in [0, k) and does not affect the others. */
int proqa_kmeans_assign_device(proqa_kmeans* h, const void* x_f16_dev, int64_t n, const float* centroids_dev,
                               int metric_l2, int32_t* assign_dev, float* dist_dev, void* stream);
/* the same with a hint per point (int32 [n], may be NULL, may alias assign_dev): any centroid index -- a Lloyd loop passes
 * the assignment of its previous iteration.  The result does not depend on the hint; a good one lets the nominating pass
 * skip most of its bookkeeping (a hint out of [0, k) is ignored for that point). */
int proqa_kmeans_assign_hinted_device(proqa_kmeans* h, const void* x_f16_dev, int64_t n, const float* centroids_dev,
                                      int metric_l2, const int32_t* hint_dev, int32_t* assign_dev, float* dist_dev,
                                      void* stream);
/* centroid c = mean of its points, summed in fp32 in point order (faiss km_update_centroids);
 * counts uint32 [k]; centroids of empty clusters are left untouched */
int proqa_kmeans_update_device(proqa_kmeans* h, const void* x_f16_dev, int64_t n, const int32_t* assign_dev,
                               float* centroids_dev, uint32_t* counts_dev, void* stream);
/* faiss' rand_perm(perm, n, seed) (std::mt19937, i2 = i + rng() % (n - i)): the permutation faiss
 * uses to sub-sample the training set and to pick the initial centroids */
int proqa_rand_perm(int64_t n, int64_t seed, int32_t* perm_out);

/* ------------------------------------------------------------------------------------
 * Inverted-file index.  Replaces
 *     quantizer = faiss.IndexFlatIP(128); index = faiss.IndexIVFFlat(quantizer, 128, nlist)
 *     index.train(x); index.add(x); index.nprobe = 20; D, I = index.search(q, k)
 * at qa/online_sampler.py:75-79 and :274 (faiss 1.6.3 semantics, restated: DESIGN.md section 2.8).  The metric is L2,
 * faiss' default when IndexIVFFlat is given no metric: the nprobe lists are picked by inner product with the float32
 * centroids (the IndexFlatIP quantizer; ties to the lowest list), and inside them rows rank by squared L2 distance
 * (D ascending; exact ties to the lowest id).  A short result ends in I = -1, D = +FLT_MAX.  Training is the caller's
 * (proqa_kmeans_*); this handle takes the centroids.  Rows are fp16 in HBM, list-major: one copy of the rows
 * (256 B), |x|^2 / 2 (4 B), the id of every position and the position of every id (8 B each) -- 276 B per row.
 * Limits of this version: d = 128, 1 <= nlist <= 4096, 1 <= k <= 128, min(nprobe, nlist) <= 1024, fewer than
 * 2^32 - 1 rows.
 * ---------------------------------------------------------------------------------- */
typedef struct proqa_ivf proqa_ivf;
int proqa_ivf_create(int d, int nlist, proqa_ivf** out);
int proqa_ivf_free(proqa_ivf* h);
/* the float32 centroids [nlist, 128] (device); only while the index holds no rows */
int proqa_ivf_set_centroids(proqa_ivf* h, const float* centroids_dev);
/* float32 queries that fp16 cannot hold: rounded (allow != 0) or refused (default) */
int proqa_ivf_allow_rounding(proqa_ivf* h, int allow);
/* append n fp16 rows [n, 128] (device) with ids ntotal .. ntotal + n - 1.  Each row goes to the list of its largest inner
 * product with the centroids (proqa_kmeans_assign_device; ties to the lowest list), after the list's earlier rows, in
 * input order: several adds give the lists of one add of the concatenation.  Re-lays the index out (old and new copies
 * side by side while it runs); waits for `stream` before it returns. */
int proqa_ivf_add_device(proqa_ivf* h, const void* xb_f16_dev, int64_t n, void* stream);
/* D float32 [nq, k], I int64 [nq, k] and, if ip_dev != NULL, the inner product q.x of every returned row (float32
 * [nq, k], the bits proqa_index_search reports for that (query, row); -FLT_MAX in empty slots).  xq_dev [nq, 128]
 * PROQA_F16, or PROQA_F32 that fp16 holds (see proqa_ivf_allow_rounding).  The result does not depend on the batch:
 * a query gets the same bits alone.  D = max(fl(|q|^2) - 2 s, 0) with s = fl(q.x - fl(|x|^2 / 2)): the three terms are
 * rounded separately, so D is within a few ulps of |q|^2 + |x|^2 of the exact distance (tests/ivf_oracle.py states the
 * bound) and is clamped at 0, which a squared distance never falls below; rows rank by s, D is non-decreasing along a
 * result.  A row holding +-inf or NaN is never returned (faiss' heap takes d < FLT_MAX only): it counts as scanned, and
 * the result ends in I = -1, D = +FLT_MAX where fewer than k finite rows were probed.
 * Host round trips: ONE, the per-list query counts of the coarse step (nlist + 2 words), read before the scan is laid
 * out; the scan, merge and outputs stay on `stream`.
 * Workspace, grown on demand and kept for later calls: nq (256 + 12 nprobe' + 4) + 20 nlist + 32 W + 8 k S bytes,
 * nprobe' = min(nprobe, nlist), W the work items and S = sum over the lists of (queries probing it) x ceil(size / chunk),
 * chunk <= 32768 rows: S <= nq nprobe' ceil(max list size / 4096). */
int proqa_ivf_search_device(proqa_ivf* h, const void* xq_dev, int dtype, int64_t nq, int k, int nprobe, float* D_dev,
                            int64_t* I_dev, float* ip_dev, void* stream);
/* rows by original id (faiss reconstruct_batch): ids int64 [n] (device) -> out [n, 128] fp16 or float32; ids outside
 * [0, ntotal) give zero rows */
int proqa_ivf_reconstruct_batch_device(const proqa_ivf* h, const int64_t* ids_dev, int64_t n, void* out_dev, int out_dtype,
                                       void* stream);
int proqa_ivf_ntotal(const proqa_ivf* h, int64_t* out);
/* sizes_out int64 [nlist] (host) */
int proqa_ivf_list_sizes(const proqa_ivf* h, int64_t* sizes_out);
/* ids_out int64 [ntotal] (host): the ids of list 0 in list order, then list 1, ... (faiss invlists->get_ids) */
int proqa_ivf_list_ids(const proqa_ivf* h, int64_t* ids_out);
int proqa_ivf_reset(proqa_ivf* h);
typedef struct proqa_ivf_stats {
  int64_t nq;             /* queries of the last search */
  int64_t rows_scanned;   /* sum over its queries of the sizes of the probed lists */
  int64_t partial_lists;  /* (query, probed list, chunk) lists the scan wrote */
  int32_t nprobe;         /* lists probed per query: min(nprobe, nlist) */
  int32_t work_items;     /* scan workgroups: (list, chunk, 32 of the list's queries) */
  int32_t chunk_rows;     /* rows per chunk */
  float search_ms;        /* HIP-event time of the whole search on its stream */
  float scan_ms;          /* of the scan kernel alone */
  int32_t reserved;
} proqa_ivf_stats;
/* statistics of the last proqa_ivf_search_device call on this handle (waits for it to finish); all zero when that call
 * failed or was refused */
int proqa_ivf_search_stats(proqa_ivf* h, proqa_ivf_stats* out);

/* ------------------------------------------------------------------------------------
 * In-batch scoring: the retriever's dev metric and the forward value of its training objective.  Replaces
 *     product = torch.mm(q, c.t()); product.argmax(-1) == target; CrossEntropyLoss(product, target)
 * at retrieval/train_retriever.py:203-205 and :318-323 without forming the [nq, nc] product.
 * q [nq, 128], c [nc, 128] fp16 row-major (device, 16-byte aligned); dim must be 128.  target int32 [nq] (device): the gold
 * column of every row; NULL means target[i] = i and needs nq <= nc.  With s[i, j] the fp32-accumulated dot product (the
 * bits proqa_index_search reports for that pair), per row i, each output (device, [nq]) optional (NULL):
 *   argmax_out  the lowest j among the greatest scores (torch's product.argmax(-1) on the CPU path)
 *   max_out     max_j s[i, j]
 *   gold_out    s[i, target[i]]
 *   rank_out    #{j : s[i, j] > gold} + #{j < target[i] : s[i, j] == gold}; 0 = correct
 *   lse_out     log sum_j exp(s[i, j]), the maximum subtracted as torch.logsumexp does; lse - gold is the row's
 *               CrossEntropyLoss
 * Non-finite scores follow torch: a NaN is greater than every number (and equal to another NaN), the first NaN wins the
 * argmax, and such a row has max = lse = NaN; a row holding +inf has lse = +inf, a row of -inf has lse = -inf.  A
 * target[i] outside [0, nc) gives gold = NaN and rank = -1 for that row.  nq == 0 succeeds and does nothing; nc == 0 with
 * nq > 0 is refused, and so are more than 2^24 rows on either side.  Enqueued on `stream`, no host synchronisation.
 * Small nq splits the columns over several workgroups per row tile through a per-device workspace (640 KiB) allocated
 * by the first such call and kept: no allocation afterwards.  Such calls of one device are ordered on the device: a
 * call on another stream than the previous one makes its stream wait (hipStreamWaitEvent) for that call's last kernel.
 * ---------------------------------------------------------------------------------- */
int proqa_inbatch_eval_f16(const void* q, const void* c, const int32_t* target, int nq, int nc, int dim,
                           int32_t* argmax_out, int32_t* rank_out, float* max_out, float* gold_out, float* lse_out,
                           void* stream);

/* ------------------------------------------------------------------------------------
 * Answer pre-filter of the matched-paragraph file (qa/prepro_dense.py:126-158, process_ground_paras): which of a question's
 * retrieved passages can hold one of its answer aliases at all.  The reference tokenises every (question, passage) pair;
 * here the FOLDED passage texts (NFD, lower-cased, final sigma -> sigma, UTF-8: the caller folds them, once) live in HBM and
 * the device runs the substring test of proqa_amd.eval_retrieval._may_match on the rows a search left on the device.
 *
 * Text store.  blob_host: blob_bytes of folded text; spans_host int64 [rows, 2]: first byte and end of every row's text in
 * the blob (rows may share a span: that text is stored once; spans may touch or overlap).  The texts are copied to the
 * current device, each distinct span at a multiple of 16 bytes and zero-padded to the next, so the kernel's 16-byte loads
 * stay inside the allocation; bytes outside a row's span never count as its text.  rows < 2^31, a text < 2 GiB, 64 GiB of
 * padded text at most.  Arguments are validated before the device is touched.
 * ---------------------------------------------------------------------------------- */
typedef struct proqa_textstore proqa_textstore;
int proqa_textstore_create(const void* blob_host, int64_t blob_bytes, const int64_t* spans_host, int64_t rows,
                           proqa_textstore** out);
int proqa_textstore_destroy(proqa_textstore* store);
/* rows of the store and the bytes its (de-duplicated, padded) texts take in HBM; either pointer may be NULL */
int proqa_textstore_info(const proqa_textstore* store, int64_t* rows, int64_t* device_text_bytes);
/* Needle table of nq questions (host arrays; validated, packed and uploaded here: the one call that allocates and waits).
 *   token_bytes, token_off int64 [n_tokens + 1]      the folded tokens of all questions, back to back, and their offsets
 *   question_token_off int64 [nq + 1]                question q owns the DISTINCT tokens [off[q], off[q + 1])
 *   alias_tokens int32, alias_off int64 [n_aliases + 1]   alias a needs the tokens alias_tokens[alias_off[a] .. alias_off[a + 1]),
 *                                                    indexes into ITS QUESTION's tokens (order and repeats do not matter)
 *   question_alias_off int64 [nq + 1]                question q owns the aliases [off[q], off[q + 1])
 * Limits (PROQA_EINVAL, checked before the device is touched): a token has 1..255 bytes; a question has at most 128 distinct
 * tokens, 64 aliases and 4096 token bytes; nq < 2^24. */
typedef struct proqa_text_needles proqa_text_needles;
int proqa_text_needles_create(const void* token_bytes, const int64_t* token_off, const int64_t* question_token_off,
                              const int32_t* alias_tokens, const int64_t* alias_off, const int64_t* question_alias_off,
                              int64_t nq, proqa_text_needles** out);
int proqa_text_needles_destroy(proqa_text_needles* needles);
/* ids_dev int64 [nq, k] (device; what proqa_index_search_device returns: -1 = empty slot), 1 <= k <= 16384, nq = the
 * table's.  mask_out uint32 [nq, ceil(k / 32)] (device): bit (j & 31) of word j / 32 of row q is set iff ids[q, j] is a row of
 * the store and some alias of question q has every one of its tokens as a byte substring of that row's text -- an alias
 * without tokens matches every row, a question without aliases none; bits at or past k are 0.  count_out int32 [nq] (device,
 * optional): the set bits of each row.  Enqueued on `stream`: no allocation, no host wait; plain stores only (a wave owns a
 * whole mask word), so the result is the same bits on every run. */
int proqa_text_prefilter(const proqa_textstore* store, const proqa_text_needles* needles, const int64_t* ids_dev, int64_t nq,
                         int k, uint32_t* mask_out, int32_t* count_out, void* stream);

/* ------------------------------------------------------------------------------------
 * .npy index files.  Replace np.save (retrieval/get_embed.py:139) and np.load
 * (retrieval/eval_retrieval.py:99-100) for 2-D C-order '<f2' / '<f4' arrays, format v1.0,
 * header padded so that data starts at a multiple of 64 bytes.
 * ---------------------------------------------------------------------------------- */
typedef struct proqa_npy_info {
  int64_t rows;
  int64_t cols;
  int32_t dtype;        /* PROQA_F16 / PROQA_F32 */
  int64_t data_offset;  /* byte offset of element [0,0] */
} proqa_npy_info;

int proqa_npy_stat(const char* path, proqa_npy_info* info);
/* read rows [row0, row0+n) into dst (host), element type as stored */
int proqa_npy_read_rows(const char* path, int64_t row0, int64_t n, void* dst, size_t dst_bytes);
/* write a whole array */
int proqa_npy_write(const char* path, const void* data, int64_t rows, int64_t cols, int dtype);
/* create a pre-sized file (header + zero-filled data) that ranks later fill by row range */
int proqa_npy_create(const char* path, int64_t rows, int64_t cols, int dtype);
/* src: n rows of `cols` elements of `dtype`; both must match the file's header (a rank writing float32 rows into a
 * '<f2' file is refused) */
int proqa_npy_write_rows(const char* path, int64_t row0, int64_t n, const void* src, int64_t cols, int dtype);

/* ------------------------------------------------------------------------------------
 * WordPiece tokenisation on the host, native and multi-threaded: `tokenizer.encode(sent, max_length=L)` of
 * retrieval/datasets.py:285-286 (transformers' BertTokenizer: clean-up, CJK spacing, NFD + accent stripping + lower-casing
 * for uncased models, punctuation splitting, greedy WordPiece) for every text of the Basic Multilingual Plane without a
 * '[', table-driven (csrc/wordpiece_tables.inc, generated from the tokenizers library), so that get_embed.py's loader does
 * not depend on ~3.5 k passages/s per thread of Python-bound tokenizer calls.  The few other texts are flagged and left to
 * the caller's reference tokenizer.
 * ---------------------------------------------------------------------------------- */
typedef struct proqa_wordpiece proqa_wordpiece;
/* vocab: the tokens of vocab.txt joined by '\n' (token i has id i), vocab_bytes long; do_lower_case: bit 0 as the model's,
 * bit 1 = ASCII only (every text with a byte >= 0x80 is flagged -1: for callers whose reference tokenizer is NOT the
 * tokenizers library the tables were generated from -- the pure-Python BertTokenizer lower-cases whole strings (final sigma),
 * NFC-normalises first and carries its own Unicode data version) */
int proqa_wordpiece_create(const char* vocab, size_t vocab_bytes, int do_lower_case, proqa_wordpiece** out);
int proqa_wordpiece_free(proqa_wordpiece* tok);
/* texts[i] (text_bytes[i] bytes, UTF-8, not NUL-terminated) -> ids_out[i, 0..max_length) = [CLS] pieces [SEP] truncated
 * to max_length, zero-padded; lens_out[i] = its length, or -1 if text i is left to the caller's reference tokenizer (a '[',
 * a character beyond the Basic Multilingual Plane, one of 15 reordering-sensitive marks, malformed UTF-8; row i of ids_out
 * is then unspecified).  n_threads host threads share the batch. */
int proqa_wordpiece_encode_batch(const proqa_wordpiece* tok, const char* const* texts, const int64_t* text_bytes, int64_t n,
                                 int max_length, int64_t* ids_out, int32_t* lens_out, int n_threads);
/* The same straight from the records of the JSON-lines input file (retrieval/datasets.py:271-283: json.loads(line) and
 * sample['text'] / sample['question']): lines[i] (line_bytes[i] bytes, surrounding white space allowed) is one JSON object,
 * the string value of its top-level member `key` (NUL-terminated) is tokenised.  lens_out[i] = -2 for a record this parser
 * does not take -- anything but a flat object of strings, numbers and true / false / null, a surrogate escape, a missing or
 * non-string member, any deviation from the JSON grammar: the caller's json module reads (or rejects) those lines. */
int proqa_wordpiece_encode_jsonl_batch(const proqa_wordpiece* tok, const char* const* lines, const int64_t* line_bytes,
                                       int64_t n, const char* key, int max_length, int64_t* ids_out, int32_t* lens_out,
                                       int n_threads);

/* ------------------------------------------------------------------------------------
 * Multi-GPU search without PyTorch (BASELINE.json configs[3]).  One process (or thread)
 * per GPU holds rows [lo, hi) of the corpus in its own proqa_index and all queries.  A sharded search is the
 * local exact top-k with global ids, ONE RCCL all-gather of the per-rank [nq, k] (id, score) lists over xGMI,
 * and the merge of proqa_topk_merge_device: bit-identical to searching the whole corpus on one GPU.
 * The reference has no such call (its search is single-process faiss, retrieval/eval_retrieval.py:102-104; its
 * one NCCL touch point is the process-group init of retrieval/get_embed.py:44-52).
 * RCCL is bound at run time (dlopen); in a PyTorch process the RCCL PyTorch loaded is used.
 * ---------------------------------------------------------------------------------- */
#define PROQA_COMM_ID_BYTES 128
typedef struct proqa_comm proqa_comm;
/* rank 0: make a unique id (ncclGetUniqueId) and hand its 128 bytes to every rank by any side channel */
int proqa_comm_get_unique_id(void* id_out);
/* every rank, with its GPU current (hipSetDevice): collective ncclCommInitRank */
int proqa_comm_create(const void* id, int world_size, int rank, proqa_comm** out);
int proqa_comm_info(const proqa_comm* comm, int* world_size, int* rank);
int proqa_comm_free(proqa_comm* comm);
/* every rank calls with the SAME queries (device pointers), nq, dtype and k, and with idx_offset = its first global
 * row; ranks must hold ascending row ranges in rank order.  D_dev / I_dev [nq, k] receive the merged result on every
 * rank.  The collective runs even for world_size 1.  The local search, the all-gather and the merge are enqueued back to
 * back (proqa_index_search_begin_device) and the host waits once, at the end; each rank's block carries a status word, so
 * that a rank whose lists overflowed triggers ONE more exchange on every rank, and a rank whose local search fails still
 * enters the collective: every rank then returns an error instead of waiting for it forever.  One stream per communicator
 * at a time (the exchange buffers belong to the communicator). */
int proqa_sharded_search_device(proqa_index* idx, proqa_comm* comm, const void* xq_dev, int64_t nq, int dtype,
                                int k, int64_t idx_offset, float* D_dev, int64_t* I_dev, void* stream);
/* The pieces of that call for a caller that brings its own collective (proqa_amd.index.ShardedIndexFlatIP over
 * torch.distributed): the per-rank block the all-gather exchanges is [ids int64 nq*k | scores float nq*k | status word],
 * every part padded to 16 bytes (_block_layout); the rank-local search writes ids, scores and the status word straight
 * into its block (proqa_index_search_begin_device), and _merge_gathered merges the n_parts blocks of the receive buffer
 * where they lie and drops every block's status word into status_host (n_parts words of PINNED host memory, e.g.
 * hipHostMalloc; read them after synchronising the stream; NULL skips it): 0 = that rank's list stands, 1 = it is being
 * rewritten by proqa_index_search_finish (exchange once more), 0xFFFFFFFF = that rank failed. */
int proqa_sharded_block_layout(int64_t nq, int k, size_t* ids_bytes, size_t* scores_bytes, size_t* block_bytes);
int proqa_topk_merge_gathered_device(const void* gathered_dev, int n_parts, int64_t nq, int k, uint32_t* status_host,
                                     float* D_dev, int64_t* I_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Measured ceilings of this GPU (bench.py "peak_measured"; SURVEY.md section 8d asks for them next to the spec
 * peaks): a 16-byte-per-lane stream over device memory and a register-resident 32x32x16 fp16 MFMA loop.
 * ---------------------------------------------------------------------------------- */
/* kind 0: copy buf[0,bytes) -> buf[bytes,2*bytes), read+written bytes counted; kind 1: read buf[0,bytes).
 * Best of `reps` launches in GB/s. */
int proqa_microbench_stream(void* buf_dev, size_t bytes, int kind, int reps, void* stream, double* gbs);
/* launches of about ms_target milliseconds; zero_operands != 0 feeds all-zero inputs (the sustained clock depends on
 * the operand bits).  Dense TFLOP/s. */
int proqa_microbench_mfma(double ms_target, int zero_operands, void* stream, double* tflops);
/* the same loop on v_mfma_i32_32x32x32_i8 (the nomination scan's instruction); dense TOP/s */
int proqa_microbench_mfma_i8(double ms_target, int zero_operands, void* stream, double* tops);
/* the same with the instruction shape as an argument: 0 = v_mfma_i32_32x32x32_i8 (the nomination scan's), 1 =
 * v_mfma_i32_16x16x64_i8 (the shape MI355X_MICROARCH.md quotes its int8 ceiling for) */
int proqa_microbench_mfma_i8_shape(double ms_target, int zero_operands, int shape, void* stream, double* tops);
/* what VALU work beside the matrix instructions costs: the int8 rate (random operands) of a loop of 8 x
 * v_mfma_i32_32x32x32_i8 + n_valu x v_xad_u32 per wave and trip, four waves per SIMD (the shape of mips_filter_i8's unit);
 * n_valu in {0, 8, 16, 24, 32, 48, 64} */
int proqa_microbench_mfma_i8_valu(double ms_target, int n_valu, void* stream, double* tops);
/* the same with the PLACEMENT of the VALU work as an argument, n_valu in {0, 16, 24, 32}: placement 0 = behind the eight
 * interleaved MFMAs (the loop above); placement 1 = the two chains of four one after the other, behind every MFMA n_valu / 8
 * instructions of the examination (v_max3_i32 tree, then v_xad_u32) of the OTHER chain's accumulators */
int proqa_microbench_mfma_i8_valu_placed(double ms_target, int n_valu, int placement, void* stream, double* tops);
/* microseconds of ONE cooperative launch of `grid` 256-thread workgroups that meet at n_syncs grid-wide barriers
 * (hipLaunchCooperativeKernel + cooperative_groups::grid_group::sync): what fusing dependent small kernels would pay */
int proqa_microbench_grid_sync(int grid, int n_syncs, void* stream, double* us);

#ifdef __cplusplus
}
#endif
#endif /* PROQA_HIP_H */
