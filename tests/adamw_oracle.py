"""The fused optimizer step (proqa_amd/optim.py, include/proqa_hip.h proqa_adamw_step) restated with torch on the CPU.

`oracle_step(..., dtype=torch.float64)` is the specification: unscale, global norm, clip coefficient, skip rule, both
update rules, loss-scale update, everything in float64.
`dtype=torch.float32` follows the arithmetic of what the reference's loop calls: apex's unscale (g * (1 / scale) in fp32),
clip_grad_norm_ (per-tensor fp32 norms, the norm of the norms, fp32 coefficient, g *= coef) and the element formulas of
transformers.AdamW / torch.optim.AdamW as in-place fp32 tensor operations.  Its distance from the float64 mode is the
yardstick of the GPU tests (tests/test_optim_gpu.py): measure_reference_error().
"""
import math

import torch

from proqa_amd import _lib

CHUNK = _lib.ADAMW_CHUNK
DYNAMIC_INIT_SCALE = 65536.0


def new_state(loss_scale=None):
    scale = 1.0 if loss_scale is None else DYNAMIC_INIT_SCALE if loss_scale == "dynamic" else float(loss_scale)
    return {"step": 0, "scale": scale, "clean_steps": 0, "skipped_steps": 0}


def hyper(betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, loss_scale=None, growth_interval=2000, torch_semantics=False,
          backoff_factor=0.5, growth_factor=2.0):
    return dict(betas=betas, eps=eps, max_grad_norm=max_grad_norm, loss_scale=loss_scale, growth_interval=growth_interval,
                torch_semantics=torch_semantics, backoff_factor=backoff_factor, growth_factor=growth_factor)


def oracle_step(state, hp, params, grads, ms, vs, lrs, wds, dtype=torch.float64):
    """One step from (state, params, ms, vs) with `grads` (scaled by state['scale']; None = no gradient).  Nothing is
    modified: returns (new_state, new_params, new_ms, new_vs, info) with info = {'norm', 'found_inf', 'clip'}; tensors
    come back in `dtype`."""
    state = dict(state)
    plain = hp["max_grad_norm"] is None and hp["loss_scale"] is None
    scale = state["scale"]
    live = [i for i, g in enumerate(grads) if g is not None]
    if dtype == torch.float64:
        ug = {i: grads[i].double() / scale for i in live}
        norm = math.sqrt(sum(float((u * u).sum()) for u in ug.values()))
        clip = 1.0
        if hp["max_grad_norm"] is not None:
            clip = min(1.0, hp["max_grad_norm"] / (norm + 1e-6))
        found_inf = not math.isfinite(norm)
        if clip != 1.0 and not found_inf:
            ug = {i: u * clip for i, u in ug.items()}
    else:
        ug = {i: grads[i].float() * (1.0 / scale) for i in live}
        norms = [torch.linalg.vector_norm(u, 2.0) for u in ug.values()]
        total = torch.linalg.vector_norm(torch.stack(norms), 2.0) if norms else torch.zeros((), dtype=torch.float32)
        norm = float(total)
        found_inf = not math.isfinite(norm)
        clip = 1.0
        if hp["max_grad_norm"] is not None:
            coef = torch.clamp(hp["max_grad_norm"] / (total + 1e-6), max=1.0)
            clip = float(coef)
            if not found_inf:
                ug = {i: u * coef for i, u in ug.items()}
    info = {"norm": norm, "found_inf": found_inf and not plain, "clip": clip}
    new_p = [p.to(dtype).clone() for p in params]
    new_m = [m.to(dtype).clone() for m in ms]
    new_v = [v.to(dtype).clone() for v in vs]
    dynamic = hp["loss_scale"] == "dynamic"
    if info["found_inf"]:
        state["skipped_steps"] += 1
        if dynamic:
            state["scale"] = scale * hp["backoff_factor"]
            state["clean_steps"] = 0
        return state, new_p, new_m, new_v, info
    state["step"] += 1
    if dynamic:
        state["clean_steps"] += 1
        if state["clean_steps"] >= hp["growth_interval"]:
            state["scale"] = scale * hp["growth_factor"]
            state["clean_steps"] = 0
    t = state["step"]
    beta1, beta2 = hp["betas"]
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    for i in live:
        g, p, m, v, lr, wd = ug[i], new_p[i], new_m[i], new_v[i], lrs[i], wds[i]
        m.mul_(beta1).add_(g, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
        if hp["torch_semantics"]:
            p.mul_(1.0 - lr * wd)
            denom = (v.sqrt() / math.sqrt(bc2)).add_(hp["eps"])
            p.addcdiv_(m, denom, value=-(lr / bc1))
        else:
            denom = v.sqrt().add_(hp["eps"])
            p.addcdiv_(m, denom, value=-(lr * math.sqrt(bc2) / bc1))
            if wd > 0.0:
                p.add_(p, alpha=-lr * wd)
    return state, new_p, new_m, new_v, info


# ---- the case set of the GPU tests ----------------------------------------------------------------------------------
LR = 1e-3
GROUP_WD = (0.01, 0.0)
CASE_SHAPES = [("one", (1,)), ("three", (3,)), ("seven", (7,)), ("v128", (128,)), ("v768", (768,)),
               ("chunk_minus_1", (CHUNK - 1,)), ("chunk", (CHUNK,)), ("chunk_plus_1", (CHUNK + 1,)),
               ("two_chunks_5", (2 * CHUNK + 5,)), ("table", (120, 128)), ("big", (300_000,)), ("empty", (0,)),
               ("slice", (4099,)), ("nograd", (64,))]
NAMES = [n for n, _ in CASE_SHAPES]
GROUP_OF = {name: i % 2 for i, name in enumerate(NAMES)}      # two groups: weight decay 0.01 and 0


def case_params(seed=0):
    """name -> fp32 CPU tensor, N(0, 0.02)"""
    gen = torch.Generator().manual_seed(1000 + seed)
    return {name: torch.randn(shape, generator=gen) * 0.02 for name, shape in CASE_SHAPES}


def case_grads(step, scale, seed=0):
    """name -> fp32 CPU gradient of step `step`, N(0, 0.01) x scale; None for 'nograd'"""
    gen = torch.Generator().manual_seed(77_000 + 100 * seed + step)
    out = {}
    for name, shape in CASE_SHAPES:
        g = torch.randn(shape, generator=gen) * 0.01 * scale
        out[name] = None if name == "nograd" else g
    return out


def rel_err(got, ref):
    """max|got - ref| / max|ref| in float64 (0 for two empty or two all-zero tensors)"""
    got, ref = got.double(), ref.double()
    if ref.numel() == 0:
        return 0.0
    diff, top = float((got - ref).abs().max()), float(ref.abs().max())
    if diff == 0.0:
        return 0.0
    return diff / top if top > 0.0 else float("inf")


def step_errors(before_p, got, ref):
    """The GPU tests' measures of one step: got / ref = (params, ms, vs) lists after the step from the same state.
    Returns {'p', 'm', 'v', 'dp'}: the maximum over the tensors of rel_err; dp is the update p_after - p_before, both
    differences taken in float64."""
    out = {"p": 0.0, "m": 0.0, "v": 0.0, "dp": 0.0}
    for i in range(len(before_p)):
        out["p"] = max(out["p"], rel_err(got[0][i], ref[0][i]))
        out["m"] = max(out["m"], rel_err(got[1][i], ref[1][i]))
        out["v"] = max(out["v"], rel_err(got[2][i], ref[2][i]))
        b = before_p[i].double()
        out["dp"] = max(out["dp"], rel_err(got[0][i].double() - b, ref[0][i].double() - b))
    return out


ACCURACY_CONFIGS = [(mgn, ls, ts) for ts in (False, True)
                    for mgn, ls in ((None, 65536.0), (1.0, 65536.0), (1e9, 65536.0), (None, None))]
ACCURACY_STEPS = 5

# measure_reference_error() on the CPU: the fp32 mode against float64 under the GPU tests' protocol, maximum over
# ACCURACY_CONFIGS, steps and tensors.  tests/test_optim_host.py checks that the function still gives these figures; the
# GPU tests allow 4 x each.
MEASURED_FP32_ERROR = {"p": 1.09e-7, "m": 1.57e-6, "v": 2.88e-6, "dp": 8.43e-6, "norm": 1.33e-6}
TOLERANCE_FACTOR = 4.0


def measure_reference_error(configs=None):
    """Run the fp32 mode along its own trajectory; before every step take its p, m, v, do one float64 step from exactly
    that state, compare.  Returns {'p', 'm', 'v', 'dp', 'norm'} (maxima) and the per-config figures."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "dp": 0.0, "norm": 0.0}
    per_config = {}
    lrs = [LR] * len(NAMES)
    wds = [GROUP_WD[GROUP_OF[n]] for n in NAMES]
    for mgn, ls, ts in (configs or ACCURACY_CONFIGS):
        hp = hyper(max_grad_norm=mgn, loss_scale=ls, torch_semantics=ts)
        state = new_state(ls)
        params = [case_params()[n] for n in NAMES]
        ms = [torch.zeros_like(p) for p in params]
        vs = [torch.zeros_like(p) for p in params]
        here = {"p": 0.0, "m": 0.0, "v": 0.0, "dp": 0.0, "norm": 0.0}
        for step in range(ACCURACY_STEPS):
            grads = [case_grads(step, state["scale"])[n] for n in NAMES]
            _, rp, rm, rv, rinfo = oracle_step(state, hp, params, grads, ms, vs, lrs, wds, torch.float64)
            state, gp, gm, gv, ginfo = oracle_step(state, hp, params, grads, ms, vs, lrs, wds, torch.float32)
            e = step_errors(params, (gp, gm, gv), (rp, rm, rv))
            e["norm"] = abs(ginfo["norm"] - rinfo["norm"]) / rinfo["norm"]
            for k, x in e.items():
                here[k] = max(here[k], x)
            params, ms, vs = gp, gm, gv
        per_config[(mgn, ls, ts)] = here
        for k, x in here.items():
            worst[k] = max(worst[k], x)
    return worst, per_config
