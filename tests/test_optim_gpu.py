"""proqa_amd.optim.FusedAdamW on the GPU against tests/adamw_oracle.py.

Case set (adamw_oracle.CASE_SHAPES, C = the chunk one workgroup owns, 16384): tensors of 1, 3, 7, 128, 768, C-1, C, C+1 and
2C+5 elements, a [120, 128] table, one of 300 000, one of 0, one whose parameter and gradient are [1:] slices of larger
buffers (4-byte but not 16-byte aligned: the scalar path) and one whose grad stays None; two groups (weight decay 0.01 and
0), lr 1e-3, parameters N(0, 0.02), gradients N(0, 0.01) x the loss scale (unscaled norm about 6.3).

Accuracy protocol: before every step the GPU's own p, m, v are copied to the host, one float64 oracle step is taken from
exactly that state, and the GPU's p, m, v after its step are compared: max|gpu - ref| / max|ref| per tensor, the maximum
over the tensors; the update dp = p_after - p_before the same way (both differences in float64); last_grad_norm relatively.
Five steps, both semantics, (max_grad_norm, loss_scale) in {(None, 2^16), (1.0, 2^16): clips, (1e9, 2^16): does not,
(None, None): the single-launch path}.

Tolerance: the rule of tests/test_train_ops_gpu.py, four times the same measure of the oracle's fp32 mode (the arithmetic
of apex's unscale, clip_grad_norm_ and the AdamW classes in fp32 on the CPU) against float64, the maximum over the
configurations; adamw_oracle.measure_reference_error(), checked by tests/test_optim_host.py.  The clipped runs carry the
fp32 norm's error into m and v, which sets those two bounds.

    measure    measured    allowed
    p          1.09e-07    4.36e-07
    m          1.57e-06    6.28e-06
    v          2.88e-06    1.15e-05
    dp         8.43e-06    3.37e-05
    norm       1.33e-06    5.32e-06
"""
import pytest
import torch

import adamw_oracle as oracle

pytestmark = pytest.mark.gpu

NAMES = oracle.NAMES
BOUNDS = {k: oracle.TOLERANCE_FACTOR * v for k, v in oracle.MEASURED_FP32_ERROR.items()}
SCALE = 65536.0


class Case:
    """The case set on the device with a FusedAdamW over it."""

    def __init__(self, dev, init=None, **kw):
        from proqa_amd.optim import FusedAdamW
        self.dev = dev
        init = oracle.case_params() if init is None else init
        self.params = {}
        for name in NAMES:
            t = init[name].float()
            if name == "slice":
                buf = torch.zeros(t.numel() + 1, device=dev)
                buf[1:] = t.to(dev)
                p = torch.nn.Parameter(buf[1:])
                assert p.data_ptr() % 16 == 4 and p.is_contiguous()
            else:
                p = torch.nn.Parameter(t.to(dev))
            self.params[name] = p
        groups = [{"params": [self.params[n] for n in NAMES if oracle.GROUP_OF[n] == g], "weight_decay": oracle.GROUP_WD[g]}
                  for g in (0, 1)]
        self.opt = FusedAdamW(groups, lr=oracle.LR, **kw)
        self.lrs = [oracle.LR] * len(NAMES)
        self.wds = [oracle.GROUP_WD[oracle.GROUP_OF[n]] for n in NAMES]

    def set_grads(self, grads):
        """fresh device tensors (the storage moves from step to step); the 'slice' gradient is misaligned as well"""
        for name, g in grads.items():
            if g is None:
                self.params[name].grad = None
            elif name == "slice":
                buf = torch.zeros(g.numel() + 1, device=self.dev)
                buf[1:] = g.to(self.dev)
                self.params[name].grad = buf[1:]
            else:
                self.params[name].grad = g.to(self.dev)

    def host(self):
        """(p, m, v) lists on the host in NAMES order"""
        st = self.opt.state
        return ([self.params[n].detach().cpu() for n in NAMES], [st[self.params[n]]["exp_avg"].cpu() for n in NAMES],
                [st[self.params[n]]["exp_avg_sq"].cpu() for n in NAMES])

    def scale(self):
        return float(self.opt.loss_scale_tensor)


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for ta, tb in zip(a, b) for x, y in zip(ta, tb))


def run_steps(dev, steps=oracle.ACCURACY_STEPS, bad_at=None, **kw):
    """`steps` calls of step() on seeded gradients (scaled by the optimizer's current scale; call `bad_at` carries one inf);
    returns (case, [norm bits per call])"""
    case = Case(dev, **kw)
    norms = []
    for k in range(steps):
        grads = oracle.case_grads(k, case.scale())
        if k == bad_at:
            grads["seven"][3] = float("inf")
        case.set_grads(grads)
        case.opt.step()
        norms.append(case.opt.last_grad_norm.cpu().view(torch.int32).item())
        case.opt.zero_grad()
    return case, norms


@pytest.mark.parametrize("max_grad_norm,loss_scale,torch_semantics", oracle.ACCURACY_CONFIGS)
def test_five_steps_match_the_float64_oracle(gpu_device, max_grad_norm, loss_scale, torch_semantics):
    hp = oracle.hyper(max_grad_norm=max_grad_norm, loss_scale=loss_scale, torch_semantics=torch_semantics)
    case = Case(gpu_device, max_grad_norm=max_grad_norm, loss_scale=loss_scale, torch_semantics=torch_semantics)
    state = oracle.new_state(loss_scale)
    worst = {k: 0.0 for k in BOUNDS}
    for k in range(oracle.ACCURACY_STEPS):
        grads = oracle.case_grads(k, state["scale"])
        p0, m0, v0 = case.host()
        state, rp, rm, rv, info = oracle.oracle_step(state, hp, p0, [grads[n] for n in NAMES], m0, v0, case.lrs, case.wds)
        case.set_grads(grads)
        case.opt.step()
        got = case.host()
        errs = oracle.step_errors(p0, got, (rp, rm, rv))
        if loss_scale is not None or max_grad_norm is not None:
            errs["norm"] = abs(float(case.opt.last_grad_norm) - info["norm"]) / info["norm"]
            assert (float(case.opt.last_clip_coef) < 1.0) == (max_grad_norm == 1.0) == (info["clip"] < 1.0)
        for key, e in errs.items():
            worst[key] = max(worst[key], e)
        # the tensor without a gradient and the empty one are left alone
        i = NAMES.index("nograd")
        assert torch.equal(got[0][i], p0[i]) and not got[1][i].any() and not got[2][i].any()
        case.opt.zero_grad()
    print({k: f"{e:.3e} / {BOUNDS[k]:.3e}" for k, e in worst.items()})
    for key, e in worst.items():
        assert e <= BOUNDS[key], (key, e, BOUNDS[key])
    fused = case.opt.state_dict()["fused"]
    assert fused["step"] == oracle.ACCURACY_STEPS and fused["skipped_steps"] == 0
    assert fused["loss_scale"] == (1.0 if loss_scale is None else loss_scale)


@pytest.mark.parametrize("torch_semantics", [False, True])
def test_a_clip_that_does_not_bite_changes_no_bit(gpu_device, torch_semantics):
    a, norms_a = run_steps(gpu_device, max_grad_norm=1e9, loss_scale=SCALE, torch_semantics=torch_semantics)
    b, norms_b = run_steps(gpu_device, max_grad_norm=None, loss_scale=SCALE, torch_semantics=torch_semantics)
    assert float(a.opt.last_clip_coef) == 1.0 and float(b.opt.last_clip_coef) == 1.0
    assert same_bits(a.host(), b.host()) and norms_a == norms_b
    assert 5.0 < float(a.opt.last_grad_norm) < 8.0


@pytest.mark.parametrize("where", ["seven", "big"])
@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_an_overflowing_step_is_skipped(gpu_device, where, value):
    case = Case(gpu_device, max_grad_norm=1.0, loss_scale="dynamic", growth_interval=2)
    opt = case.opt
    assert case.scale() == 65536.0
    grads = oracle.case_grads(0, 65536.0)
    grads[where][grads[where].numel() // 2] = value
    before = case.host()
    case.set_grads(grads)
    opt.step()
    assert same_bits(case.host(), before)
    assert int(opt.step_tensor) == 0 and int(opt.skipped_steps) == 1 and case.scale() == 32768.0
    assert not torch.isfinite(opt.last_grad_norm).item()
    # the next clean step updates; the scale doubles after two clean steps and not after one
    opt.zero_grad()
    case.set_grads(oracle.case_grads(1, 32768.0))
    opt.step()
    after = case.host()
    for i, n in enumerate(NAMES):
        changed = not torch.equal(after[0][i], before[0][i])
        assert changed == (n not in ("empty", "nograd")), n
    assert int(opt.step_tensor) == 1 and int(opt.skipped_steps) == 1 and case.scale() == 32768.0
    opt.zero_grad()
    case.set_grads(oracle.case_grads(2, 32768.0))
    opt.step()
    assert int(opt.step_tensor) == 2 and case.scale() == 65536.0
    assert opt.state_dict()["fused"] == {"step": 2, "skipped_steps": 1, "clean_steps": 0, "loss_scale": 65536.0}


def test_a_fixed_scale_never_changes(gpu_device):
    case = Case(gpu_device, loss_scale=1024.0, growth_interval=1)
    grads = oracle.case_grads(0, 1024.0)
    grads["big"][17] = float("inf")
    before = case.host()
    case.set_grads(grads)
    case.opt.step()
    assert same_bits(case.host(), before) and int(case.opt.skipped_steps) == 1 and case.scale() == 1024.0
    for k in (1, 2, 3):
        case.set_grads(oracle.case_grads(k, 1024.0))
        case.opt.step()
        assert case.scale() == 1024.0
    assert int(case.opt.step_tensor) == 3 and not same_bits(case.host(), before)


def test_gradient_storage_may_move_or_stay(gpu_device):
    kw = dict(max_grad_norm=1.0, loss_scale=SCALE)
    moved, keep_alive = Case(gpu_device, **kw), []
    stayed = Case(gpu_device, **kw)
    for k in range(3):
        grads = oracle.case_grads(k, SCALE)
        moved.set_grads(grads)
        keep_alive.append([p.grad for p in moved.params.values()])        # so that the next step's storage is elsewhere
        if k:
            assert moved.params["big"].grad.data_ptr() != keep_alive[-2][NAMES.index("big")].data_ptr()
        moved.opt.step()
        moved.opt.zero_grad(set_to_none=True)
        if k == 0:
            stayed.set_grads(grads)
        else:
            for n, g in grads.items():
                if g is not None:
                    assert stayed.params[n].grad is not None
                    stayed.params[n].grad.copy_(g)
        stayed.opt.step()
        stayed.opt.zero_grad(set_to_none=False)
    assert same_bits(moved.host(), stayed.host())


def test_accumulated_gradients_equal_their_sum(gpu_device):
    kw = dict(max_grad_norm=1.0, loss_scale=SCALE)
    two, one = Case(gpu_device, **kw), Case(gpu_device, **kw)
    g1, g2 = oracle.case_grads(0, SCALE), oracle.case_grads(1, SCALE)
    two.set_grads(g1)
    for n, g in g2.items():
        if g is not None:
            two.params[n].grad += g.to(gpu_device)        # what a second backward() does
    one.set_grads(g1)
    summed = {n: None if g is None else one.params[n].grad + g2[n].to(gpu_device) for n, g in g1.items()}
    for n, g in summed.items():
        one.params[n].grad = g
    two.opt.step()
    one.opt.step()
    assert same_bits(two.host(), one.host())
    assert float(two.opt.last_grad_norm) == float(one.opt.last_grad_norm) > 8.0      # sqrt(2) x the single norm


def test_two_runs_are_bit_identical(gpu_device):
    kw = dict(max_grad_norm=1.0, loss_scale="dynamic", growth_interval=2, bad_at=1)
    a, norms_a = run_steps(gpu_device, **kw)
    b, norms_b = run_steps(gpu_device, **kw)
    assert same_bits(a.host(), b.host()) and norms_a == norms_b
    assert a.opt.state_dict()["fused"] == b.opt.state_dict()["fused"]


def test_checkpoint_resumes_bit_for_bit(gpu_device):
    kw = dict(max_grad_norm=1.0, loss_scale="dynamic", growth_interval=2)
    straight, _ = run_steps(gpu_device, steps=5, bad_at=1, **kw)
    first, _ = run_steps(gpu_device, steps=3, bad_at=1, **kw)
    sd = first.opt.state_dict()
    assert sd["fused"] == {"step": 2, "skipped_steps": 1, "clean_steps": 1, "loss_scale": 32768.0}
    assert set(sd["state"][0]) == {"exp_avg", "exp_avg_sq"} and len(sd["state"]) == len(NAMES)
    p, _, _ = first.host()
    resumed = Case(gpu_device, init=dict(zip(NAMES, p)), **kw)
    resumed.opt.load_state_dict(sd)
    for k in (3, 4):
        resumed.set_grads(oracle.case_grads(k, resumed.scale()))
        resumed.opt.step()
        resumed.opt.zero_grad()
    assert same_bits(resumed.host(), straight.host())
    assert resumed.opt.state_dict()["fused"] == straight.opt.state_dict()["fused"]
    assert straight.opt.state_dict()["fused"] == {"step": 4, "skipped_steps": 1, "clean_steps": 1, "loss_scale": 65536.0}
    with pytest.raises(ValueError, match="fused"):
        resumed.opt.load_state_dict({k: v for k, v in sd.items() if k != "fused"})


@pytest.mark.parametrize("kw", [dict(max_grad_norm=1.0, loss_scale="dynamic"), dict()], ids=["full", "plain"])
def test_step_never_waits_for_the_device(gpu_device, kw):
    case = Case(gpu_device, **kw)
    case.set_grads(oracle.case_grads(0, case.scale()))
    case.opt.step()                      # (first use: pinned staging memory is allocated)
    case.set_grads(oracle.case_grads(1, case.scale()))
    loss = torch.ones((), device=gpu_device)
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        scaled = case.opt.scale_loss(loss)
        case.opt.step()
        case.opt.zero_grad()
        norm, scale, skipped = case.opt.last_grad_norm, case.opt.loss_scale_tensor, case.opt.skipped_steps
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert norm.is_cuda and scale.is_cuda and skipped.is_cuda and scaled.is_cuda
    assert float(scaled) == (65536.0 if kw else 1.0)


def test_under_grad_scaler_an_overflowing_step_is_skipped(gpu_device):
    """tests/test_trainable_gpu.py::test_grad_scaler_skips_an_overflowing_step with FusedAdamW as the optimizer"""
    from proqa_amd.optim import FusedAdamW
    from proqa_amd.trainable import inbatch_loss
    from test_trainable_gpu import make_model, on, reference
    sd, batch, *_ = reference()
    model = make_model(gpu_device, sd)
    dev_batch = on(gpu_device, batch)
    opt = FusedAdamW(model.parameters(), lr=1e-3, eps=1e-8, weight_decay=0.0, torch_semantics=True)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40, backoff_factor=2.0 ** -30, growth_interval=1000)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for step in range(2):
        out = model(dev_batch)
        loss = inbatch_loss(out["q"], out["c"])
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 2.0)
        scaler.step(opt)
        scaler.update()
        torch.cuda.synchronize()
        changed = any(not torch.equal(before[k], v) for k, v in model.state_dict().items())
        if step == 0:
            assert not changed and scaler.get_scale() == 2.0 ** 10 and opt.state_dict()["fused"]["step"] == 0
        else:
            assert changed and all(torch.isfinite(v).all() for v in model.state_dict().values())
            assert opt.state_dict()["fused"]["step"] == 1


@pytest.mark.parametrize("kw", [dict(loss_scale=1024.0, torch_semantics=True), dict(loss_scale="dynamic", torch_semantics=False)],
                         ids=["torch-fixed", "reference-dynamic"])
def test_the_towers_train_with_it(gpu_device, tmp_path, kw):
    """The training condition of tests/test_trainable_gpu.py with the fused step in the loop."""
    from proqa_amd.optim import FusedAdamW
    from proqa_amd.retriever import BertForRetriever
    from proqa_amd.trainable import inbatch_loss
    from test_encoder_gpu import TOL_GOLDEN
    from test_trainable_gpu import CFG, in_batch_accuracy, make_model, on, reference
    sd, batch, *_ = reference()
    model = make_model(gpu_device, sd)
    dev_batch = on(gpu_device, batch)
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_grad_norm=2.0, **kw)
    first = None
    for _ in range(20):
        out = model(dev_batch)
        loss = inbatch_loss(out["q"], out["c"])
        if first is None:
            first = loss.item()
        opt.scale_loss(loss).backward()
        opt.step()
        opt.zero_grad()
    with torch.no_grad():
        out = model(dev_batch)
        final = inbatch_loss(out["q"], out["c"]).item()
    print("loss: start", first, "after 20", final, opt.state_dict()["fused"])
    assert abs(first - 2.08) < 0.05
    assert final <= 0.2
    if kw["torch_semantics"]:
        assert in_batch_accuracy(out["q"], out["c"]) == 8
        path = tmp_path / "checkpoint_best.pt"
        torch.save(model.state_dict(), path)
        loaded = torch.load(path, map_location="cpu")
        assert list(loaded) == list(sd) and all(v.dtype == torch.float32 for v in loaded.values())
        infer = BertForRetriever(CFG, device=gpu_device)
        infer.load_state_dict(loaded)
        emb = {"q": infer.get_embed({"input_ids": dev_batch["input_ids_q"], "input_mask": dev_batch["input_mask_q"]}, True)["embed"],
               "c": infer.get_embed({"input_ids": dev_batch["input_ids_c"], "input_mask": dev_batch["input_mask_c"]}, False)["embed"]}
        for k in ("q", "c"):
            assert (emb[k].float() - out[k].float()).abs().max().item() < TOL_GOLDEN
        assert in_batch_accuracy(emb["q"], emb["c"]) == 8
