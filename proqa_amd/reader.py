"""Reader of BertRetrieveQA (qa/bert_retrieve_qa.py) for --do_predict on MI355X.

    reader = BertReader.load(checkpoint, config, device)
    out = reader.forward(batch)   # start, end (positions in the sequence), span_score, select[, logits]
    out = reader.forward(batch, n_best=20)   # + nbest_start / nbest_end / nbest_score [B, 20], span_lse [B, 2]

The reader's BertModel runs in libproqa_hip.so (`proqa_encoder_forward_hidden`: token-type embeddings, every layer for
every token, last hidden state in the packed [T, hidden] layout, tanh pooler), and `proqa_reader_span_f16` turns the
hidden states into start / end logits and the best span of every sequence in one launch, without the reference's
[B, L, L] span-score tensor.  The question tower (retriever.bert_q + proj_q of the same checkpoint) is the retriever's
BertForRetriever.  Weights are fp16, accumulation fp32, as everywhere in this package; there is no CPU path.
"""
import torch

from . import _lib
from .retriever import BertForRetriever, _Tower, config_from_dict, random_state_dict as _retriever_random_state_dict
from .retriever import tower_keys

MAX_ANSWER_LEN = 10     # hard-coded in the reference's predict (train_retrieve_qa.py:301); --max_answer_len is ignored there


def _strip_module(sd):
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


class BertReader:
    """Inference-only BertRetrieveQA: reader tower + qa_outputs (+ select_outputs) + the question tower."""

    def __init__(self, config, device=None):
        self.config = config if not isinstance(config, dict) else config_from_dict(config)
        self._lib = _lib.load()
        _lib.require_gpu()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.tower = None
        self.retriever = None
        self.add_select = False
        self.max_answer_len = MAX_ANSWER_LEN

    @classmethod
    def load(cls, checkpoint, config, device=None):
        """checkpoint: a path to a torch state_dict of BertRetrieveQA, or the dict itself ('module.' prefixes tolerated)."""
        sd = torch.load(checkpoint, map_location="cpu") if isinstance(checkpoint, str) else checkpoint
        return cls(config, device).load_state_dict(sd)

    def load_state_dict(self, state_dict):
        sd = {k: v for k, v in _strip_module(state_dict).items() if not k.endswith("position_ids")}
        cfg = self.config
        want = tower_keys("bert", cfg.num_hidden_layers) + ["qa_outputs.weight", "qa_outputs.bias"]
        want += tower_keys("retriever.bert_q", cfg.num_hidden_layers) + ["retriever.proj_q.weight", "retriever.proj_q.bias"]
        missing = [k for k in want if k not in sd]
        if missing:
            raise RuntimeError(f"Error(s) in loading state_dict for BertReader: missing keys {missing[:8]}"
                               f"{'...' if len(missing) > 8 else ''}")

        def dev16(name):
            return sd[name].detach().to(device=self.device, dtype=torch.float16).contiguous()

        self.tower = _Tower(sd, "bert", None, cfg, self.device)
        self.type_table = dev16("bert.embeddings.token_type_embeddings.weight")     # [n_types, H]
        self.qa_w = dev16("qa_outputs.weight")                                       # [2, H]
        self.qa_b = dev16("qa_outputs.bias")
        self.add_select = "select_outputs.weight" in sd
        if self.add_select:
            self.select_w = dev16("select_outputs.weight").reshape(-1).contiguous()  # [H]
            self.select_b = dev16("select_outputs.bias")
        # the question tower alone: the passage tower of the checkpoint is not needed for prediction
        self.retriever = BertForRetriever(cfg, device=self.device).load_query_tower(sd, "retriever.bert_q", "retriever.proj_q")
        return self

    @torch.no_grad()
    def hidden(self, input_ids, segment_ids, seq_lens, want_pooled=False):
        """Packed last hidden state [T, H] fp16 (sequence b from row cu_seqlens[b]) and the pooled [B, H] (or None).
        input_ids / segment_ids: [B, L] int64 right-padded (CUDA); seq_lens: host list of the valid lengths."""
        B, L = input_ids.shape
        H = self.config.hidden_size
        T = int(sum(seq_lens))
        if min(seq_lens) < 1:
            raise ValueError("every sequence needs at least one token")
        hid = torch.empty((T, H), dtype=torch.float16, device=self.device)
        pooled = torch.empty((B, H), dtype=torch.float16, device=self.device) if want_pooled else None
        lens = torch.tensor(seq_lens, dtype=torch.int32).to(self.device)
        ids = input_ids.to(self.device, torch.int64).contiguous()
        seg = segment_ids.to(self.device, torch.int64).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.proqa_encoder_forward_hidden(
                self.tower._handle, ids.data_ptr(), seg.data_ptr(), self.type_table.data_ptr(), self.type_table.shape[0],
                lens.data_ptr(), B, L, T, _lib.ENC_PACKED, hid.data_ptr(), pooled.data_ptr() if pooled is not None else None,
                _lib.current_stream_ptr()))
        return hid, pooled

    @torch.no_grad()
    def span(self, hidden, seq_lens, para_offset, max_len, return_logits=False, padded=False, n_best=None):
        """proqa_reader_span_f16 over packed hidden states (padded=True: hidden is [B * max_len, H])
        -> (start int32 [B], end int32 [B], score fp32 [B], logits fp16 [rows, 2] or None), on the device.
        n_best > 0: proqa_reader_span_nbest_f16 instead, and a fifth element dict(nbest_start, nbest_end int32 [B, N],
        nbest_score fp32 [B, N], span_lse fp32 [B, 2]); start / end / score are then views of column 0."""
        B = len(seq_lens)
        dev = self.device
        lens = torch.tensor(seq_lens, dtype=torch.int32)
        cu = torch.zeros(B + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(lens, 0)
        lens, cu = lens.to(dev), cu.to(dev)
        po = torch.tensor(para_offset, dtype=torch.int32).to(dev)
        logits = torch.zeros((hidden.shape[0], 2), dtype=torch.float16, device=dev) if return_logits else None
        layout = (hidden.data_ptr(), lens.data_ptr() if padded else None, None if padded else cu.data_ptr(), B, int(max_len),
                  hidden.shape[1], po.data_ptr(), self.qa_w.data_ptr(), self.qa_b.data_ptr(), int(self.max_answer_len))
        logits_ptr = logits.data_ptr() if logits is not None else None
        if n_best:
            N = int(n_best)
            nb_start = torch.empty((B, N), dtype=torch.int32, device=dev)
            nb_end = torch.empty((B, N), dtype=torch.int32, device=dev)
            nb_score = torch.empty((B, N), dtype=torch.float32, device=dev)
            lse = torch.empty((B, 2), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(self._lib.proqa_reader_span_nbest_f16(
                    *layout, N, nb_start.data_ptr(), nb_end.data_ptr(), nb_score.data_ptr(), lse.data_ptr(), logits_ptr,
                    _lib.current_stream_ptr()))
            nbest = {"nbest_start": nb_start, "nbest_end": nb_end, "nbest_score": nb_score, "span_lse": lse}
            return nb_start[:, 0], nb_end[:, 0], nb_score[:, 0], logits, nbest
        start = torch.empty(B, dtype=torch.int32, device=dev)
        end = torch.empty(B, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.proqa_reader_span_f16(*layout, start.data_ptr(), end.data_ptr(), score.data_ptr(), logits_ptr,
                                                       _lib.current_stream_ptr()))
        return start, end, score, logits

    @torch.no_grad()
    def forward(self, batch, return_logits=False, n_best=0):
        """batch: input_ids, segment_ids ([B, L] int64), seq_lens (host list), para_offset (host list)
        -> dict(start, end: int32 positions in the sequence (-1: no paragraph token), span_score fp32,
                select fp32 [B] (select_outputs on the pooled output; None without it), logits [T, 2] fp16 packed
                (return_logits), cu_seqlens (host list)).
        n_best > 0 adds nbest_start / nbest_end int32 [B, N], nbest_score fp32 [B, N] (score descending, then start, then
        end ascending; missing entries -1, -1, -inf) and span_lse fp32 [B, 2] (the log-sum-exp of the paragraph's start /
        end logits); start / end / span_score are then column 0."""
        if self.tower is None:
            raise RuntimeError("load_state_dict must be called before forward")
        ids = batch["input_ids"]
        seq_lens = [int(x) for x in batch["seq_lens"]]
        hid, pooled = self.hidden(ids, batch["segment_ids"], seq_lens, want_pooled=self.add_select)
        start, end, score, logits, *nbest = self.span(hid, seq_lens, batch["para_offset"], ids.shape[1], return_logits,
                                                      n_best=n_best)
        select = None
        if self.add_select:
            select = torch.empty(len(seq_lens), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self._lib.proqa_reader_select_f16(pooled.data_ptr(), len(seq_lens), self.config.hidden_size,
                                                             self.select_w.data_ptr(), self.select_b.data_ptr(),
                                                             select.data_ptr(), _lib.current_stream_ptr()))
        cu = [0]
        for n in seq_lens:
            cu.append(cu[-1] + n)
        out = {"start": start, "end": end, "span_score": score, "select": select, "logits": logits, "cu_seqlens": cu}
        if nbest:
            out.update(nbest[0])
        return out

    __call__ = forward


def random_state_dict(config, seed=0, std=0.02, add_select=False):
    """N(0, std) weights in BertRetrieveQA's layout (tests, timing): bert.*, qa_outputs.*, retriever.{bert_q,bert_c,
    proj_q,proj_c}.* and, with add_select, select_outputs.*"""
    cfg = config if not isinstance(config, dict) else config_from_dict(config)
    sd = {f"retriever.{k}": v for k, v in _retriever_random_state_dict(cfg, seed=seed, std=std).items()}
    other = _retriever_random_state_dict(cfg, seed=seed + 1, std=std)
    sd.update({"bert." + k[len("bert_q."):]: v for k, v in other.items() if k.startswith("bert_q.")})
    g = torch.Generator().manual_seed(seed + 2)
    H = cfg.hidden_size
    sd["qa_outputs.weight"] = std * torch.randn((2, H), generator=g)
    sd["qa_outputs.bias"] = std * torch.randn((2,), generator=g)
    if add_select:
        sd["select_outputs.weight"] = std * torch.randn((1, H), generator=g)
        sd["select_outputs.bias"] = std * torch.randn((1,), generator=g)
    return sd
