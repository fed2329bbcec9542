"""The matched-paragraph file of reader training: for every training question, which of its top-k retrieved passages hold
the answer.

Drop-in for /root/reference/qa/prepro_dense.py:process_ground_paras (:126-158): the same positional arguments, the same
printed coverage (`np.mean(topk_covered)`) and the same output, one JSON line per question = the raw item plus
"matched_paras": {para_id: matched} -- the first match's untokenised text (match="string") or the de-duplicated list of
regex matches (match="regex"), json.dumps defaults.  train_reader.py --matched-para-path reads that file.

    python prepro_dense.py --raw-data nq-train.txt --index-path para_embed.npy --query-embed nq-train-query.npy \
        --index2paraid idx_id.json --text-sidecar idx_id.txt --save-path nq_ft_train_matched.txt [--topk 10000]

Where the candidates come from: `retrieved` (the reference's file of {"para_id": [...]} lines; ids are mapped to index rows
through the inverted id map, an unknown id is a ValueError), or, with retrieved=None, the top-k search here, in batches of
questions whose id lists stay on the device.

Routes of match="string":
  prefilter="device"  the folded texts of the corpus are uploaded once (textstore.TextStore), text_prefilter marks the slots
                      whose passage can hold an alias at all (eval_retrieval._may_match, bit for bit), the rows of the marked
                      slots alone come back, and the host pool confirms each with para_has_answer(..., return_matched=True)
                      on the sidecar text.  A question beyond the kernel's limits (textstore.within_limits) takes the host
                      route and is counted.
  prefilter="host"    every candidate goes to the pool, which applies _may_match before it tokenises: the yardstick.
match="regex" (TREC) has no pre-filter: every candidate goes to the host regex_match, as in the reference.

Deviations from the reference: lines are written in input order (its imap_unordered order is arbitrary); regex matches are
sorted (qa_utils.match_answer_span; its list(set(...)) order changes from run to run); the passage texts come from the index's
text sidecar by row, or from `db_path` by id (host routes only) instead of the hard-coded '../data/nq_paras.db'; find_span
(commented out there) and debug() are not restated.  The worker pool is forked before the library touches the GPU.
"""
import argparse
import json
import os
import time
from multiprocessing import Pool as ProcessPool

import numpy as np

from . import eval_retrieval as ev
from .qa_utils import match_answer_span
from .utils import normalize

QUESTION_BATCH = 512       # questions per search + pre-filter call: [512, 10000] int64 ids = 41 MB on the device
LAST_RUN_STATS = {}        # filled by process_ground_paras: seconds per stage and counts of the last run


def _text_of(row, para_id):
    if ev.PROCESS_TEXTS is not None and row >= 0:
        return ev.PROCESS_TEXTS[row]
    return ev.PROCESS_DB.get_doc_text(para_id)


def _needles_worker(answer):
    """the words of every alias, as para_has_answer forms them"""
    return [ev._words(alias) for alias in answer]


def _match_worker(task):
    """(answer, needles or None, rows, para_ids, match, screen) -> (matched_paras items in candidate order, survivors).
    screen: apply _may_match here and count its survivors (the host route); otherwise the rows are survivors already."""
    answer, needles, rows, para_ids, match, screen = task
    items, survivors = [], 0
    if match == "regex":
        for row, para_id in zip(rows, para_ids):
            matched = match_answer_span(normalize(_text_of(row, para_id)), answer, None, "regex")   # regex_match, sorted
            if len(matched) > 0:
                items.append((para_id, matched))
        return items, len(rows)
    if needles is None:
        needles = _needles_worker(answer)
    folded = [[ev._fold(t) for t in needle] for needle in needles]
    for row, para_id in zip(rows, para_ids):
        text = _text_of(row, para_id)
        if screen and not ev._may_match(folded, ev._fold(normalize(text))):
            continue
        survivors += 1
        covered, matched = ev.para_has_answer(answer, text, True, needles=needles)
        if covered:
            items.append((para_id, matched))
    return items, survivors


def _load_id_map(index2paraid):
    """row -> para id as a list"""
    if index2paraid.endswith(".ids"):
        from .gen_index_id_map import SidecarMap
        m = SidecarMap(index2paraid)
        return m.take(np.arange(len(m)))
    with open(index2paraid) as f:
        idx_id = json.load(f)
    return [idx_id[str(i)] for i in range(len(idx_id))]


def _rows_of(retrieved, k, row_ids):
    """the `para_id` lists of the retrieved file as rows [nq, k] (-1 = no candidate) through the inverted id map"""
    inverse = {}
    for row, para_id in enumerate(row_ids):
        inverse.setdefault(para_id, row)
    width = max([min(len(r["para_id"]), k) for r in retrieved] + [1])
    rows = np.full((len(retrieved), width), -1, dtype=np.int64)
    for q, r in enumerate(retrieved):
        for j, para_id in enumerate(r["para_id"][:k]):
            row = inverse.get(para_id)
            if row is None and isinstance(para_id, str):
                row = inverse.get(normalize(para_id))
            if row is None:
                raise ValueError(f"question {q}: retrieved para_id {para_id!r} is not in the index's id map")
            rows[q, j] = row
    return rows


def _surviving_rows(ids, mask, counts):
    """(ids int64 [nq, k], mask int32 [nq, words], counts int32 [nq]) on the device -> per question the rows of its marked
    slots, in slot order, on the host: only the survivors cross the bus."""
    import torch
    nq, k = ids.shape
    shifts = torch.arange(32, device=ids.device, dtype=torch.int32)
    marked = ((mask.unsqueeze(-1) >> shifts) & 1).reshape(nq, -1)[:, :k].bool()
    rows = ids[marked].cpu().numpy()
    ends = np.cumsum(counts.cpu().numpy().astype(np.int64))
    assert len(rows) == (ends[-1] if nq else 0), "count_out disagrees with the mask"
    return [rows[e - c:e] for e, c in zip(ends, np.diff(ends, prepend=0))]


def process_ground_paras(retrieved="../data/wq_finetuneq_train_10000.txt", save_path="../data/wq_ft_train_matched.txt",
                         raw_data="../data/wq-train.txt", num_workers=40, debug=False, k=10000, match="string", *,
                         index_path=None, query_embeds=None, index2paraid=None, text_sidecar=None, db_path=None,
                         prefilter="device"):
    if match not in ("string", "regex"):
        raise ValueError(f"match must be 'string' or 'regex', got {match!r}")
    if prefilter not in ("device", "host"):
        raise ValueError(f"prefilter must be 'device' or 'host', got {prefilter!r}")
    use_device = match == "string" and prefilter == "device"
    searching = retrieved is None
    if searching and not (index_path and query_embeds and index2paraid):
        raise ValueError("without a retrieved file the search needs index_path, query_embeds and index2paraid")
    if text_sidecar is None and index2paraid:
        from .gen_index_id_map import text_sidecar_of
        text_sidecar = text_sidecar_of(index2paraid)
    if (use_device or searching) and not text_sidecar:
        raise ValueError("the device pre-filter and the search here read the passage texts by row: text_sidecar is needed "
                         "(gen_index_id_map --texts)")
    if not text_sidecar and not db_path:
        raise ValueError("no passage texts: give text_sidecar (texts by index row) or db_path (texts by para id)")
    if text_sidecar and not index2paraid:
        raise ValueError("text_sidecar addresses the texts by index row: index2paraid is needed to name the rows")
    stats = dict(match=match, prefilter=prefilter if match == "string" else "none", k=int(k), workers=int(num_workers))
    t_start = time.perf_counter()
    with open(raw_data) as f:
        raw = [json.loads(line) for line in f.readlines()]
    if not searching:
        with open(retrieved) as f:
            retrieved = [json.loads(line) for line in f.readlines()]
        if len(retrieved) != len(raw):
            raise ValueError(f"{len(retrieved)} retrieved lines for {len(raw)} questions")
    answers = [item["answer"] for item in raw]
    nq = len(raw)

    # every host worker is forked here, before the library touches the GPU (num_workers < 1: no pool, the calling process
    # does the host work itself)
    initializer, initargs = (ev.init, [db_path, text_sidecar]) if db_path else (_init_texts_only, [text_sidecar])
    pool = ProcessPool(processes=num_workers, initializer=initializer, initargs=initargs) if num_workers >= 1 else \
        _InProcess(initializer, initargs)
    store = index = None
    try:
        row_ids = _load_id_map(index2paraid) if index2paraid else None
        # [nq, <=k] candidate rows when they come from the retrieved file and the texts are read by row
        rows_host = _rows_of(retrieved, k, row_ids) if not searching and text_sidecar else None
        stats["setup_seconds"] = time.perf_counter() - t_start      # inputs, pool fork, id map
        t0 = time.perf_counter()
        needles = pool.map(_needles_worker, answers, chunksize=64) if match == "string" else [None] * nq
        stats["needles_seconds"] = time.perf_counter() - t0

        if use_device:
            from . import textstore
            folded = [textstore.fold_needles(n) for n in needles]
            on_device = [textstore.within_limits(f) for f in folded]
            store = textstore.TextStore.from_sidecar(text_sidecar, pool=pool)
            stats.update(fold_seconds=store.fold_seconds, upload_seconds=store.upload_seconds,
                         store_text_bytes=store.device_text_bytes)
        else:
            on_device = [False] * nq
        stats["host_route_questions"] = int(nq - sum(on_device)) if match == "string" else 0

        xq = None
        t0 = time.perf_counter()
        if searching:
            from . import npy
            from .index import IndexFlatIP
            info = npy.stat(index_path)
            index = IndexFlatIP(128, capacity=info["rows"])
            index.add_npy(index_path, 0, info["rows"])
            xq = npy.load(query_embeds)
            if xq.shape[0] != nq:
                raise ValueError(f"{xq.shape[0]} query embeddings for {nq} questions")
        if searching or use_device:
            import torch
            torch.cuda.synchronize()      # (PyTorch's own start-up on the device is not a stage of either route)
        stats["index_load_seconds"] = time.perf_counter() - t0

        search_s = prefilter_s = confirm_s = 0.0
        candidates = survivors = 0
        results = [None] * nq
        for q0 in range(0, nq, QUESTION_BATCH):
            q1 = min(q0 + QUESTION_BATCH, nq)
            ids_dev = ids_host = None
            if searching or use_device:
                import torch
                t0 = time.perf_counter()
                if searching:
                    _D, ids_dev = index.search_device(torch.from_numpy(np.ascontiguousarray(xq[q0:q1])).cuda(), int(k))
                else:
                    ids_dev = torch.from_numpy(rows_host[q0:q1]).cuda()
                torch.cuda.synchronize()
                search_s += time.perf_counter() - t0
            surviving = [None] * (q1 - q0)
            if use_device:
                t0 = time.perf_counter()
                table = textstore.NeedleTable([f if ok else [] for f, ok in zip(folded[q0:q1], on_device[q0:q1])])
                mask, counts = store.prefilter(ids_dev, table)
                surviving = _surviving_rows(ids_dev, mask, counts)
                filled = (ids_dev >= 0).sum(1).cpu().numpy()
                table.close()
                prefilter_s += time.perf_counter() - t0
            if ids_dev is not None and not all(on_device[q0:q1]):
                ids_host = ids_dev.cpu().numpy()          # the host routes read the whole lists
            elif ids_dev is None:
                ids_host = rows_host[q0:q1] if rows_host is not None else None
            t0 = time.perf_counter()
            tasks = []
            for q in range(q0, q1):
                if on_device[q]:
                    rows = surviving[q - q0]
                    n_cand = int(filled[q - q0])
                    para_ids = [row_ids[int(r)] for r in rows]
                elif ids_host is not None:
                    rows = ids_host[q - q0]
                    rows = rows[rows >= 0]
                    n_cand = len(rows)
                    para_ids = [row_ids[int(r)] for r in rows] if searching else list(retrieved[q]["para_id"][:k])
                else:       # texts by para id from the DB: no rows
                    para_ids = list(retrieved[q]["para_id"][:k])
                    rows = [-1] * len(para_ids)
                    n_cand = len(para_ids)
                candidates += n_cand
                tasks.append((answers[q], needles[q], [int(r) for r in rows], para_ids, match, not on_device[q]))
            for q, (items, n_surv) in zip(range(q0, q1), pool.imap(_match_worker, tasks, chunksize=4)):
                survivors += n_surv
                results[q] = dict(items)
            confirm_s += time.perf_counter() - t0
    finally:
        pool.close()
        pool.join()
        if store is not None:
            store.close()
        if index is not None:
            index.close()

    for item, matched in zip(raw, results):
        item["matched_paras"] = matched
    topk_covered = [len(r["matched_paras"]) > 0 for r in raw]
    print(np.mean(topk_covered))
    t0 = time.perf_counter()
    if not debug:
        with open(save_path, "w") as g:
            for item in raw:
                g.write(json.dumps(item) + "\n")
    stats.update(questions=nq, search_seconds=search_s, prefilter_seconds=prefilter_s, confirm_seconds=confirm_s,
                 write_seconds=time.perf_counter() - t0, candidates=int(candidates), survivors=int(survivors),
                 confirmed=int(sum(len(r["matched_paras"]) for r in raw)), total_seconds=time.perf_counter() - t_start)
    LAST_RUN_STATS.clear()
    LAST_RUN_STATS.update(stats)
    if os.environ.get("PROQA_STATS_JSON"):
        with open(os.environ["PROQA_STATS_JSON"], "w") as f:
            json.dump(LAST_RUN_STATS, f)


class _InProcess:
    """The pool's interface over the calling process (num_workers < 1); the scorer's per-process state is put back at the end."""

    def __init__(self, initializer, initargs):
        self._saved = (ev.PROCESS_TOK, ev.PROCESS_DB, ev.PROCESS_TEXTS)
        initializer(*initargs)

    def map(self, fn, items, chunksize=None):
        return [fn(item) for item in items]

    imap = map

    def close(self):
        ev.PROCESS_TOK, ev.PROCESS_DB, ev.PROCESS_TEXTS = self._saved

    def join(self):
        pass


def _init_texts_only(text_sidecar):
    """per-worker state without a sqlite DB: the tokenizer and the text sidecar"""
    from .basic_tokenizer import SimpleTokenizer
    from .gen_index_id_map import TextSidecar
    ev.PROCESS_TOK = SimpleTokenizer()
    ev.PROCESS_DB = None
    ev.PROCESS_TEXTS = TextSidecar(text_sidecar)


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--raw-data", type=str, default=None, help="QA JSON-lines ({question, answer})")
    parser.add_argument("--save-path", type=str, default=None, help="the matched-paragraph file to write")
    parser.add_argument("--retrieved", type=str, default=None,
                        help="JSON-lines of {para_id: [...]} per question (the reference's input); default: search here")
    parser.add_argument("--index-path", type=str, default=None, help="passage embeddings (.npy)")
    parser.add_argument("--query-embed", type=str, default=None, help="question embeddings (.npy), one row per raw-data line")
    parser.add_argument("--index2paraid", type=str, default=None, help="idx_id.json or its .ids sidecar")
    parser.add_argument("--text-sidecar", type=str, default=None, help="<stem>.txt of gen_index_id_map --texts")
    parser.add_argument("--db-path", type=str, default=None, help="sqlite DB of the passages (texts by id; host routes only)")
    parser.add_argument("--topk", type=int, default=10000)
    parser.add_argument("--match", choices=("string", "regex"), default="string")
    parser.add_argument("--prefilter", choices=("device", "host"), default="device")
    parser.add_argument("--num-workers", type=int, default=40, help="host processes (0: none, this process does their work)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    required = ["raw_data", "save_path"]
    if args.retrieved is None:
        required += ["index_path", "query_embed", "index2paraid", "text_sidecar"]
    elif args.match == "string" and args.prefilter == "device":
        required += ["index2paraid", "text_sidecar"]
    for name in required:
        if not getattr(args, name):
            raise SystemExit("prepro_dense.py: --%s is required" % name.replace("_", "-"))
    for name in ("raw_data", "retrieved", "index_path", "query_embed", "index2paraid", "text_sidecar", "db_path"):
        path = getattr(args, name)
        if path and not os.path.exists(path):
            raise SystemExit("prepro_dense.py: --%s: no such file: %s" % (name.replace("_", "-"), path))
    process_ground_paras(args.retrieved, args.save_path, args.raw_data, num_workers=args.num_workers, k=args.topk,
                         match=args.match, index_path=args.index_path, query_embeds=args.query_embed,
                         index2paraid=args.index2paraid, text_sidecar=args.text_sidecar, db_path=args.db_path,
                         prefilter=args.prefilter)


if __name__ == "__main__":
    main()
