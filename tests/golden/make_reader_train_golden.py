"""Generate tests/golden/reader_train_golden.npz and reader_state_dict_keys.json by running the REFERENCE's own
BertRetrieveQA.forward in train() mode, and backward(), on CPU in float64.

Run in the build container only (needs the reference checkout and transformers; only the two files it writes travel):

    python tests/golden/make_reader_train_golden.py <path of the reference's qa/ directory>

As make_reader_loss_golden.py, the model is built without its constructor (no pretrained weights are read), but this time
nothing is a stub: `bert` is transformers.BertModel(SMALL_CONFIG) in float64, `retriever` is the reference's
BertForRetriever (also without its constructor: two BertModels and two nn.Linear), `qa_outputs` an nn.Linear, every dropout
rate 0.  The weights are proqa_amd.reader.random_state_dict(SMALL_CONFIG, seed 0), the batch is
reader_train_oracle.SMALL_READER_BATCH.  What runs is qa/bert_retrieve_qa.py:58-171 over transformers' BERT.

Recorded: the loss (shared norm and per-passage norm); for the shared-norm case every parameter's gradient L2 norm and its
values at 64 seeded positions -- the whole gradient for the small tensors (`full`: qa_outputs, the token-type table, the
LayerNorm vectors) -- and the sorted key list of the reference's state_dict().
"""
import importlib.machinery
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
sys.path.insert(0, os.path.dirname(HERE))                      # tests/: the oracle and its batch
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository: proqa_amd.reader.random_state_dict

N_SAMPLES = 64


def full(key, value):
    """tensors recorded whole: the head, the token-type table, every LayerNorm vector"""
    return key.startswith("qa_outputs.") or "token_type_embeddings" in key or "LayerNorm" in key


def sample_positions(index, numel):
    g = torch.Generator().manual_seed(7000 + index)
    return torch.randint(0, numel, (N_SAMPLES,), generator=g).numpy().astype(np.int64)


def stub_modules():
    for name in ("tensorflow", "faiss", "apex", "torch.utils.tensorboard"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            m.SummaryWriter = object
            sys.modules[name] = m
    sys.path.insert(0, REF)
    sys.path.append(os.path.join(os.path.dirname(os.path.abspath(REF)), "retrieval"))


def build_model(cfg, shared_norm):
    from transformers import BertConfig, BertModel
    from bert_retrieve_qa import BertRetrieveQA
    from retriever import BertForRetriever
    bc = BertConfig(**cfg, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = BertRetrieveQA.__new__(BertRetrieveQA)
    torch.nn.Module.__init__(model)
    model.shared_norm, model.separate, model.add_select, model.drop_early = shared_norm, False, False, False
    model.bert = BertModel(bc)
    retriever = BertForRetriever.__new__(BertForRetriever)
    torch.nn.Module.__init__(retriever)
    retriever.bert_q, retriever.bert_c = BertModel(bc), BertModel(bc)
    retriever.proj_q, retriever.proj_c = torch.nn.Linear(bc.hidden_size, 128), torch.nn.Linear(bc.hidden_size, 128)
    model.retriever = retriever
    model.qa_outputs = torch.nn.Linear(bc.hidden_size, 2)
    model.qa_drop = torch.nn.Dropout(0.0)
    return model.double().train()


def main():
    stub_modules()
    import reader_train_oracle as oracle
    from proqa_amd.reader import random_state_dict
    cfg = oracle.SMALL_CONFIG
    sd = random_state_dict(cfg, seed=0)
    b = oracle.SMALL_READER_BATCH
    batch = {k: v.clone() for k, v in b.items()}
    batch["input_mask"], batch["input_mask_q"] = b["input_mask"].long(), b["input_mask_q"].long()
    batch["para_embed"] = b["para_embed"].double()
    arrays = {}
    for shared in (True, False):
        model = build_model(cfg, shared)
        keys = sorted(model.state_dict())
        missing, unexpected = model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=False)
        assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
        loss = model(batch)["loss"]
        loss.backward()
        name = "shared" if shared else "separate"
        arrays[f"{name}::loss"] = loss.detach().double().numpy()
        print(name, float(loss.detach()))
        if not shared:
            continue
        with open(os.path.join(HERE, "reader_state_dict_keys.json"), "w") as f:
            json.dump(keys, f, indent=0)
            f.write("\n")
        for index, (key, p) in enumerate(sorted(model.named_parameters())):
            g = torch.zeros_like(p) if p.grad is None else p.grad
            arrays[f"norm::{key}"] = g.norm().numpy()
            if full(key, g):
                arrays[f"full::{key}"] = g.numpy()
            else:
                at = sample_positions(index, g.numel())
                arrays[f"at::{key}"] = at
                arrays[f"values::{key}"] = g.reshape(-1).numpy()[at]
    np.savez_compressed(os.path.join(HERE, "reader_train_golden.npz"), **arrays)


if __name__ == "__main__":
    main()
