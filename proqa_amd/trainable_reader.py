"""Trainable reader on MI355X: BertRetrieveQA (qa/bert_retrieve_qa.py of the reference) with gradients.

`TrainableReader` is a torch.nn.Module with the parameter names of the reference's BertRetrieveQA.state_dict() -- `bert.*`
(the reader's BERT, read with segment ids), `qa_outputs.*`, and `retriever.*`, a TrainableRetriever submodule -- so the
reference's loop (qa/train_retrieve_qa.py) runs with the model class and the optimizer swapped, its sampler keeps calling
`model.retriever.get_embed`, and the checkpoint it saves loads into BertReader.load / train_retrieve_qa.py --do_predict.

forward([net_input, ...]) in train() mode is ONE pass over the questions of the list, three steps, all on the device: the
reader tower on [CLS] q [SEP] p [SEP] with token types over all their sequences (trainable.run_tower: the operators of
TrainableRetriever, the embeddings through proqa_embed_layernorm_typed_varlen_f16 and its backward), the question tower on
ROW 0 of every question's input_ids_q (the reference runs B identical rows and uses q[0]), and one call of
proqa_amd.reader_loss on the packed hidden states (reader_loss_multi; reader_loss for a pass of one).  One host round trip
per tower pass (the sizes and the checks of the masks), none in the loss.  Within an accumulation window no weight changes,
so a pass is the optimisation step of its questions run one after another; -> {"loss": the sum, "losses", "joint", "early":
per question}.  forward(net_input) in train() mode is the pass of that one question; -> {"loss", "joint", "early"}, scalars.

forward(net_input) in eval() mode returns the reference's keys (start_logits, end_logits, rank_logits) for its dev loop.  It
runs the INFERENCE class (proqa_amd.reader.BertReader: the fused encoder and proqa_reader_span_f16) over an fp16 copy of the
parameters, taken at the first forward after eval() is entered, so a dev score during training is the score --do_predict
gives for the checkpoint.  predict_qa keeps BertReader itself as its hot path.

Precision and dropout are TrainableRetriever's: fp32 masters, fp16 activations, fp32 sums and parameter gradients; BERT's
two rates inside the fused operators, qa_drop inside the loss kernels (site 255).  Not built: --separate and --add-select
(they need a select term in the loss kernels).  There is no CPU path.
"""
import torch

from .reader import BertReader
from .reader_loss import reader_loss, reader_loss_multi
from .retriever import config_from_dict, tower_keys
from .trainable import TrainableRetriever, _Node, _parameter_shapes, run_tower
from .trainable import state_dict_keys as _retriever_keys

CALLS_PER_FORWARD = 3      # dropout `call`s one train() forward takes: reader tower, question tower, head -- per PASS: a
                           # list of questions takes the same three as one question


def state_dict_keys(config):
    """The keys of the reference's BertRetrieveQA.state_dict() (without `position_ids` buffers), in its order, without a GPU."""
    cfg = config if not isinstance(config, dict) else config_from_dict(config)
    return (tower_keys("bert", cfg.num_hidden_layers) + ["retriever." + k for k in _retriever_keys(cfg)] +
            ["qa_outputs.weight", "qa_outputs.bias"])


_PARAGRAPH_MESSAGE = ("paragraph_mask must be one run of True per row, from the paragraph's first token to the token before "
                      "the final [SEP]")


def _paragraph_geometry(pmask, lens):
    """(para_offset int32 [B]: the first True of the row, or the row's length; a device bool: some row is not
    [para_offset, len - 1)) -- on the device, no host round trip"""
    S = pmask.shape[1]
    ar = torch.arange(S, device=pmask.device, dtype=torch.int32)[None]
    first = torch.argmax(pmask.to(torch.int8), dim=1).to(torch.int32)
    po = torch.where(pmask.any(dim=1), first, lens)
    want = (ar >= po[:, None]) & (ar < (lens[:, None] - 1))
    return po, (want != pmask).any()


def _check_rate(name, rate):
    if not 0.0 <= float(rate) <= 0.9:
        raise ValueError(f"{name}={rate!r}: a dropout rate must be in [0, 0.9]")
    return float(rate)


class TrainableReader(torch.nn.Module):
    """BertRetrieveQA with gradients.  forward(net_input) takes the sampler's net_input; train(): {"loss", "joint",
    "early"}, eval(): {"start_logits", "end_logits", "rank_logits"}; train() also takes a list of net_inputs (one pass)."""

    def __init__(self, config, device=None, *, shared_norm=True, drop_early=False, qa_drop=0.0, hidden_dropout_prob=0.0,
                 attention_probs_dropout_prob=0.0, dropout_seed=None, separate=False, add_select=False,
                 deterministic=False):
        super().__init__()
        cfg = config if not isinstance(config, dict) else config_from_dict(config)
        if separate or add_select:
            raise ValueError("TrainableReader: separate / add_select are not built: they need a select term in the loss "
                             "kernels (DESIGN.md section 3h)")
        self.qa_drop = _check_rate("qa_drop", qa_drop)
        self.hidden_dropout_prob = _check_rate("hidden_dropout_prob", hidden_dropout_prob)
        self.attention_probs_dropout_prob = _check_rate("attention_probs_dropout_prob", attention_probs_dropout_prob)
        dev = torch.device(device) if device is not None else torch.device("cuda")
        if dev.type != "cuda":
            raise RuntimeError("proqa_amd.TrainableReader runs on MI355X only; there is no CPU path")
        self.shared_norm, self.drop_early = bool(shared_norm), bool(drop_early)
        self.deterministic = bool(deterministic)     # the word-embedding gradients in a fixed order, in both towers
        self._dropout_seed = int(torch.initial_seed() if dropout_seed is None else dropout_seed) & 0xFFFFFFFFFFFFFFFF
        self._dropout_call = 0
        self._inference = None
        # the towers of the retriever (and every check of the geometry and of the device)
        retriever = TrainableRetriever(cfg, device=dev, hidden_dropout_prob=hidden_dropout_prob,
                                       attention_probs_dropout_prob=attention_probs_dropout_prob,
                                       dropout_seed=self._dropout_seed, deterministic=self.deterministic)
        dev = retriever.device
        self.config, self.device = cfg, dev
        self._flat = {}
        shapes = _parameter_shapes(cfg, tower_keys("bert", cfg.num_hidden_layers))
        shapes["qa_outputs.weight"], shapes["qa_outputs.bias"] = (2, cfg.hidden_size), (2,)
        g = torch.Generator().manual_seed(1)
        for key, shape in shapes.items():      # transformers' initialisation: N(0, 0.02), LayerNorm (1, 0), biases 0
            if key.endswith("LayerNorm.weight"):
                value = torch.ones(shape)
            elif key.endswith(".bias"):
                value = torch.zeros(shape)
            else:
                value = 0.02 * torch.randn(shape, generator=g)
            node = self
            *path, leaf = key.split(".")
            for name in path:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            p = torch.nn.Parameter(value.to(dev))
            node.register_parameter(leaf, p)
            self._flat[key] = p
            if key == "bert.pooler.dense.bias":      # the reference's order: bert, retriever, qa_outputs
                self.add_module("retriever", retriever)

    @classmethod
    def from_args(cls, config, args, device=None, **kwargs):
        """The reference's flags (qa/train_retrieve_qa.py): shared_norm, drop_early, qa_drop, separate, add_select and
        retriever_path, and this project's `deterministic`; BERT's two dropout rates come from kwargs (the reference takes them
        from the pretrained config)."""
        model = cls(config, device, shared_norm=getattr(args, "shared_norm", False), drop_early=getattr(args, "drop_early", False),
                    qa_drop=getattr(args, "qa_drop", 0.0), separate=getattr(args, "separate", False),
                    add_select=getattr(args, "add_select", False), deterministic=getattr(args, "deterministic", False),
                    **kwargs)
        if getattr(args, "retriever_path", ""):
            model.load_pretrained_retriever(args.retriever_path)
        return model

    # -- reference-compatible surface -----------------------------------------------------
    def state_dict_keys(self):
        return state_dict_keys(self.config)

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """Accepts the reference checkpoint layout: a 'module.' prefix (DataParallel) is stripped, `position_ids` buffers
        of newer transformers are ignored."""
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        sd = {k: v for k, v in sd.items() if not k.endswith("position_ids")}
        self._inference = None
        return super().load_state_dict(sd, strict=strict, **kwargs)

    def load_pretrained_retriever(self, path_or_dict):
        """BertRetrieveQA.load_pretrained_retriever: a retriever checkpoint (path or state dict) into `retriever`."""
        sd = torch.load(path_or_dict, map_location="cpu") if isinstance(path_or_dict, str) else path_or_dict
        self._inference = None
        return self.retriever.load_state_dict(sd)

    def freeze_c_encoder(self):
        for name, p in self.retriever.named_parameters():
            if name.startswith(("bert_c.", "proj_c.")):
                p.requires_grad = False

    def freeze_retriever(self):
        for p in self.retriever.parameters():
            p.requires_grad = False

    def dropout_state(self):
        """(seed, call) of the module's own masks; a train() forward with any rate above 0 advances `call` by
        CALLS_PER_FORWARD = 3: the reader tower takes call, the question tower call + 1, the head (site 255) call + 2."""
        return self._dropout_seed, self._dropout_call

    def set_dropout_state(self, state):
        seed, call = state
        self._dropout_seed, self._dropout_call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFF

    def _apply(self, fn, *args, **kwargs):
        probe = fn(torch.empty(0, dtype=torch.float32, device=self.device))
        if probe.device.type != "cuda":
            raise RuntimeError("proqa_amd.TrainableReader runs on MI355X only; there is no CPU path")
        if probe.dtype != torch.float32:
            raise RuntimeError("the parameters are the fp32 masters; the module casts them to fp16 itself")
        if probe.device != self.device:
            self.device = probe.device
        self._inference = None
        return super()._apply(fn, *args, **kwargs)

    # -- forward ----------------------------------------------------------------------------
    def train(self, mode=True):
        self._inference = None          # eval() takes its fp16 copy of the parameters again after any training
        return super().train(mode)

    def forward(self, net_input):
        if isinstance(net_input, (list, tuple)):
            return self._forward_questions(list(net_input))
        if not self.training:
            self._check_inputs(net_input)
            return self._predict(net_input, net_input["paragraph_mask"].to(torch.bool))
        out = self._forward_questions([net_input])       # one question is the shortest pass
        return {"loss": out["loss"], "joint": out["joint"][0], "early": out["early"][0]}

    @staticmethod
    def _check_inputs(x):
        ids = x["input_ids"]
        if not ids.is_cuda:
            raise RuntimeError("TrainableReader expects CUDA tensors (the reference feeds move_to_cuda(batch))")
        if ids.shape[0] == 0:
            raise ValueError("TrainableReader: an empty batch")
        if x["paragraph_mask"].shape != ids.shape:
            raise ValueError(f"paragraph_mask {tuple(x['paragraph_mask'].shape)} must have the shape of input_ids "
                             f"{tuple(ids.shape)}")

    def _forward_questions(self, batches):
        """train() mode, a list of the sampler's net_input dicts: the questions of one pass.  One reader-tower pass over all
        sequences (padded on the device to the widest batch, packed by run_tower), one question-tower pass over row 0 of
        every question's input_ids_q (the reference encodes B identical rows and uses q[0]), one loss call; two host round
        trips and one (seed, call) triple for the pass.  -> {"loss": losses.sum(), "losses" fp32 [Q] (with gradients), "joint",
        "early" fp32 [Q]}.  A pass of one question takes its tensors as they are (no copy) and the single-question loss
        entry, whose bits reader_loss_multi gives at Q = 1."""
        if not self.training:
            raise ValueError("TrainableReader: a list of questions is a training pass; eval() takes one net_input dict")
        if not batches:
            raise ValueError("TrainableReader: an empty list of questions")
        for x in batches:
            self._check_inputs(x)
            if x["para_embed"].dtype != batches[0]["para_embed"].dtype:
                raise ValueError("TrainableReader: the questions of a pass must share para_embed's dtype")

        def under(parts):                         # the questions' tensors under each other
            return parts[0] if len(parts) == 1 else torch.cat(parts, 0)

        def stacked(key, rows=None, fill=0):      # ... [n, width] tensors, padded on the right to the widest
            parts = [x[key] if rows is None else x[key][:rows] for x in batches]
            width = max(t.shape[1] for t in parts)
            return under([t if t.shape[1] == width else torch.nn.functional.pad(t, (0, width - t.shape[1]), value=fill)
                          for t in parts])

        ids, pmask = stacked("input_ids"), stacked("paragraph_mask").to(torch.bool)
        p_hid, p_att, p_qa = self.hidden_dropout_prob, self.attention_probs_dropout_prob, self.qa_drop
        seed, call = self._dropout_seed, self._dropout_call
        if p_hid > 0 or p_att > 0 or p_qa > 0:
            self._dropout_call = (call + CALLS_PER_FORWARD) & 0xFFFFFF
        geometry = {}

        def paragraph_probe(lens):
            geometry["para_offset"], bad = _paragraph_geometry(pmask, lens)
            return bad, _PARAGRAPH_MESSAGE

        hidden, cu, lens, max_len = run_tower(self._flat, "bert", self.config, ids, stacked("input_mask"),
                                              type_ids=stacked("segment_ids"), drop=(p_hid, p_att, seed, call),
                                              probe_extra=paragraph_probe, deterministic=self.deterministic)
        q = run_tower(self.retriever._flat, "bert_q", self.config, stacked("input_ids_q", rows=1),
                      stacked("input_mask_q", rows=1), proj="proj_q", drop=(p_hid, p_att, seed, (call + 1) & 0xFFFFFF),
                      deterministic=self.deterministic)
        operands = (under([x["para_embed"] for x in batches]), under([x["top5000_labels"].reshape(-1) for x in batches]),
                    stacked("start_positions", fill=-1), stacked("end_positions", fill=-1), geometry["para_offset"])
        options = dict(cu_seqlens=cu, shared_norm=self.shared_norm, early=not self.drop_early, qa_drop=p_qa,
                       dropout_state=(seed, (call + 2) & 0xFFFFFF), max_seq_len=max_len)
        w, b = self._flat["qa_outputs.weight"], self._flat["qa_outputs.bias"]
        if len(batches) == 1:       # the one branch on the pass length: the single entry takes no CSR arrays
            out = reader_loss(hidden, w, b, q[0], *operands, **options)
            return {"loss": out["loss"], "losses": out["loss"][None], "joint": out["joint"][None], "early": out["early"][None]}
        question_seq, question_para = [0], [0]
        for x in batches:
            question_seq.append(question_seq[-1] + x["input_ids"].shape[0])
            question_para.append(question_para[-1] + x["para_embed"].shape[0])
        out = reader_loss_multi(hidden, w, b, q, *operands, question_seq=question_seq, question_para=question_para, **options)
        return {"loss": out["losses"].sum(), "losses": out["losses"], "joint": out["joint"], "early": out["early"]}

    def inference_reader(self):
        """The BertReader that eval() forwards run: the inference class over an fp16 copy of the parameters, taken at the
        first use after eval() was entered (train(), a load or a move drops it).  For evaluations that drive the inference
        class themselves (predict_qa.evaluate in train_reader.py); in train() mode the copy would go stale: refused."""
        if self.training:
            raise RuntimeError("TrainableReader.inference_reader(): call eval() first; the copy is taken per evaluation")
        if self._inference is None:
            with torch.no_grad():
                self._inference = BertReader(self.config, self.device).load_state_dict(
                    {k: p.detach() for k, p in self.named_parameters()})
        return self._inference

    @torch.no_grad()
    def _predict(self, net_input, pmask):
        """eval(): the reference's keys, computed by the inference class over an fp16 copy of the parameters (taken at the
        first eval() forward after train() or a load), so that what is evaluated during training is what BertReader and
        --do_predict serve.  start / end logits [B, L] fp16 carry the bits of proqa_reader_span_f16's logits, -inf outside
        the paragraph mask; rank_logits [1, P] fp32.  One host round trip (the lengths and the checks of the masks)."""
        reader = self.inference_reader()
        dev = self.device
        ids = net_input["input_ids"]
        B, S = ids.shape
        mask = net_input["input_mask"].to(torch.bool)
        lens = mask.sum(dim=1).clamp_(min=1).to(torch.int32)
        bad = (mask[:, 1:] & ~mask[:, :-1]).any() if S > 1 else torch.zeros((), dtype=torch.bool, device=mask.device)
        po, bad_paragraph = _paragraph_geometry(pmask, lens)
        probe = torch.cat([torch.stack([bad, bad_paragraph]).to(torch.int32), lens, po]).cpu().tolist()
        if probe[0]:
            raise ValueError("input_mask must be right-padded (a prefix of True per row), as re_collate produces")
        if probe[1]:
            raise ValueError(_PARAGRAPH_MESSAGE)
        seq_lens, para_offset = probe[2:2 + B], probe[2 + B:]
        hidden, _ = reader.hidden(ids, net_input["segment_ids"], seq_lens)
        *_, logits = reader.span(hidden, seq_lens, para_offset, S, return_logits=True)
        cu = torch.zeros(B, dtype=torch.int64, device=dev)
        cu[1:] = torch.cumsum(lens[:-1], 0)
        rows = (cu[:, None] + torch.arange(S, device=dev)[None]).clamp_(max=hidden.shape[0] - 1)
        neg = torch.full((), float("-inf"), dtype=torch.float16, device=dev)
        out = torch.where(pmask[..., None], logits[rows], neg)                    # [B, S, 2]; only masked rows are kept
        q = reader.retriever.get_embed({"input_ids": net_input["input_ids_q"][:1], "input_mask": net_input["input_mask_q"][:1]},
                                       True)["embed"]
        rank = q[:1].float() @ net_input["para_embed"].to(device=dev, dtype=torch.float32).t()
        return {"start_logits": out[..., 0].contiguous(), "end_logits": out[..., 1].contiguous(), "rank_logits": rank}
