"""Generate tests/golden/reader_loss_golden.npz by running the REFERENCE's own BertRetrieveQA.forward in train() mode on CPU.

Run in the build container only (needs the reference checkout; only the .npz it writes travels):

    python tests/golden/make_reader_loss_golden.py [path of the reference's qa/ directory]

As make_reader_golden.py: modules the reference imports but the container lacks are stubbed in sys.modules.  The model is
built without its constructor (no pretrained weights are read): `bert` and `retriever.bert_q` / `proj_q` are stubs that
return given float64 leaf tensors, `qa_outputs` is a float64 nn.Linear, `qa_drop` has rate 0.  What runs is
qa/bert_retrieve_qa.py:58-171 itself, and torch.autograd gives the gradients w.r.t. the hidden states, q and qa_outputs.

Cases: {shared norm, per-sequence norm} x {answers and gold labels, answers only, gold labels only}; B 4, L 24, H 64, P 40.
"""
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/qa"

B, L, H, P, A = 4, 24, 64, 40, 3
LENS = [24, 17, 9, 6]
PARA_OFFSET = [6, 5, 4, 5]          # the last sequence has an empty paragraph: [5, 5)


def stub_modules():
    for name in ("tensorflow", "faiss", "apex", "torch.utils.tensorboard"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            m.SummaryWriter = object
            sys.modules[name] = m
    sys.path.insert(0, REF)
    sys.path.append(os.path.join(os.path.dirname(os.path.abspath(REF)), "retrieval"))


class Returns(torch.nn.Module):
    """A tower stub: whatever it is called with, it returns the given tuple."""

    def __init__(self, *out):
        super().__init__()
        self.out = out

    def forward(self, *args, **kwargs):
        return self.out


def build_model(shared_norm, hidden, q, qa_w, qa_b):
    from bert_retrieve_qa import BertRetrieveQA
    model = BertRetrieveQA.__new__(BertRetrieveQA)
    torch.nn.Module.__init__(model)
    model.shared_norm, model.separate, model.add_select, model.drop_early = shared_norm, False, False, False
    model.bert = Returns(hidden)
    model.retriever = torch.nn.Module()
    model.retriever.bert_q = Returns(None, q)
    model.retriever.proj_q = torch.nn.Identity()
    model.qa_outputs = torch.nn.Linear(H, 2).double()
    with torch.no_grad():
        model.qa_outputs.weight.copy_(qa_w)
        model.qa_outputs.bias.copy_(qa_b)
    model.qa_drop = torch.nn.Dropout(0.0)
    return model.train()


def main():
    stub_modules()
    g = torch.Generator().manual_seed(2024)
    hidden = torch.randn(B, L, H, generator=g).half().double()
    qa_w = (0.3 * torch.randn(2, H, generator=g)).half().double()
    qa_b = (0.1 * torch.randn(2, generator=g)).half().double()
    q = (0.4 * torch.randn(B, 128, generator=g)).half().double()        # B rows, as the reference forms them; row 0 counts
    para = (0.4 * torch.randn(P, 128, generator=g)).half().double()
    pmask = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        pmask[b, PARA_OFFSET[b]:LENS[b] - 1] = 1
    # answers: a duplicated pair in sequence 0, one pair in sequence 1, a pair outside the mask in sequence 2
    start = torch.tensor([[7, 7, 12], [6, -1, -1], [2, -1, -1], [-1, -1, -1]])
    end = torch.tensor([[9, 9, 12], [10, -1, -1], [5, -1, -1], [-1, -1, -1]])
    none = torch.full((B, A), -1)
    labels = torch.zeros(P, dtype=torch.long)
    labels[[1, 17, P - 1]] = 1
    kinds = {"both": (start, end, labels), "answers": (start, end, torch.zeros_like(labels)), "gold": (none, none, labels)}
    arrays = dict(hidden=hidden.numpy(), qa_w=qa_w.numpy(), qa_b=qa_b.numpy(), q=q.numpy(), para=para.numpy(),
                  lens=np.asarray(LENS), para_offset=np.asarray(PARA_OFFSET))
    for shared in (True, False):
        for kind, (s, e, lab) in kinds.items():
            h = hidden.clone().requires_grad_(True)
            qq = q.clone().requires_grad_(True)
            model = build_model(shared, h, qq, qa_w, qa_b)
            batch = {"input_ids": None, "input_mask": None, "segment_ids": None, "input_ids_q": None, "input_mask_q": None,
                     "paragraph_mask": pmask, "para_embed": para, "start_positions": s, "end_positions": e,
                     "para_targets": lab[:B], "top5000_labels": lab}
            loss = model(batch)["loss"]
            loss.backward()
            name = f"{'shared' if shared else 'separate'}_{kind}"
            arrays.update({f"{name}::start": s.numpy(), f"{name}::end": e.numpy(), f"{name}::labels": lab.numpy(),
                           f"{name}::loss": loss.detach().double().numpy(), f"{name}::d_hidden": h.grad.numpy(),
                           f"{name}::d_q": qq.grad.numpy(), f"{name}::d_qa_w": model.qa_outputs.weight.grad.numpy(),
                           f"{name}::d_qa_b": model.qa_outputs.bias.grad.numpy()})
            print(name, float(loss.detach()))
    np.savez_compressed(os.path.join(HERE, "reader_loss_golden.npz"), **arrays)


if __name__ == "__main__":
    main()
