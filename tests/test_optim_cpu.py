"""sliders_conceptmod_amd.optim (Lion, Prodigy as torch classes) on CPU tensors against the float64 restatement of
tests/optim_refs.py, under bars of 3 x dist(fp32 emulation, float64); what those bars can see (mutated restatements); the
optimiser rule of train_common; the exports of the native steps."""
import os

import numpy as np
import pytest
import torch

import optim_refs as R
from sliders_conceptmod_amd import _native, optim, train_common as TC, train_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("lion", v) for v in R.LION_VARIANTS] + [("prodigy", v) for v in R.PRODIGY_VARIANTS]


def run_torch(kind: str, n: int, variant: str, pieces: int = 1):
    """The torch class over the case's gradients, the vector cut into `pieces` parameter tensors; the history in the
    layout of the references."""
    p, grads = R.inputs(n)
    _, _, lrs, max_norm, hyper = R.reference(kind, n, variant)
    cuts = np.array_split(np.arange(n), pieces)
    params = [torch.nn.Parameter(torch.from_numpy(p[c].copy())) for c in cuts]
    opt = (optim.Lion if kind == "lion" else optim.Prodigy)(params, lr=lrs[0], **hyper)
    keys = [q for q in R.VECTORS[kind] if q not in ("p", "d")]
    hist = {q: [] for q in R.VECTORS[kind] + ("k",)}
    for g, lr in zip(grads, lrs):
        for group in opt.param_groups:
            group["lr"] = lr
        # The classes do not clip: the trainer does, in front of them.  The harness hands them the gradient as the fp32
        # emulation clips it (norm summed pairwise), so that the classes are measured and not a norm: torch's own
        # clip_grad_norm_ sums 300001 squares 8e-7 off, which alone is 9 x the bar on exp_avg (measured here).
        g = R.clip(g, max_norm, R.F32)
        for c, q in zip(cuts, params):
            q.grad = torch.from_numpy(g[c].copy())
        opt.step()
        hist["p"].append(np.concatenate([q.detach().numpy() for q in params]))
        for key in keys:
            hist[key].append(np.concatenate([opt.state[q][key].numpy() for q in params]))
        if kind == "prodigy":
            hist["d"].append(opt.d)
            hist["k"].append(opt.param_groups[0]["k"])
    return hist


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("kind,variant", CASES)
def test_torch_class_against_float64(kind, variant, n):
    got = run_torch(kind, n, variant)
    ratio, q, step = R.worst_ratio(kind, n, variant, got)
    print(f"{kind} {variant} n={n}: worst dist / bar {ratio:.3f} ({q}, step {step})")
    assert ratio <= 1.0, (ratio, q, step)
    if kind == "prodigy":
        assert got["k"] == R.reference(kind, n, variant)[0]["k"]
        if variant != "coupled_decay":  # (its first gradient is weight_decay * p, not zero: no step is skipped)
            assert got["k"] == [0] + list(range(1, R.STEPS))  # the zero first gradient: k stays 0, then counts


@pytest.mark.parametrize("n", [257, 5000])
@pytest.mark.parametrize("kind,variant", CASES)
def test_three_parameter_tensors_share_one_d(kind, variant, n):
    """The vector cut into three parameter tensors: the one-tensor result within the same bars (one d, sums over all)."""
    got = run_torch(kind, n, variant, pieces=3)
    ratio, q, step = R.worst_ratio(kind, n, variant, got)
    assert ratio <= 1.0, (ratio, q, step)


def test_lion_moves_by_exactly_lr():
    """After one Lion step every element with c != 0 sits exactly lr from its decayed value, the others on it."""
    n, lr, wd = 5000, 1e-4, 0.01
    p, grads = R.inputs(n)
    g = grads[1]
    q = torch.nn.Parameter(torch.from_numpy(p.copy()))
    q.grad = torch.from_numpy(g.copy())
    optim.Lion([q], lr=lr, weight_decay=wd).step()
    decayed = p * np.float32(1.0 - lr * wd)
    want = (decayed.astype(np.float64) - np.float64(np.float32(lr)) * np.sign(g)).astype(np.float32)  # c = 0.1 g at step 1
    assert (g == 0).sum() >= n // 13 and np.array_equal(q.detach().numpy(), want)
    assert np.array_equal(q.detach().numpy()[g == 0], decayed[g == 0])


@pytest.mark.parametrize("variant", list(R.PRODIGY_VARIANTS))
def test_prodigy_d_never_decreases(variant):
    """d is monotone although the last two gradients pull d_hat below d_max (test_bars_see_each_mutation: d_max_ignored)."""
    for n in (257, 5000):
        d = run_torch("prodigy", n, variant)["d"]
        assert all(b >= a for a, b in zip(d, d[1:])) and d[0] == 1e-6 and d[-1] > 1e-6, d
        if variant != "coupled_decay":  # the skipped step, then d_hat = 0 while p0 == p
            assert d[1] == 1e-6, d


@pytest.mark.parametrize("kind", ["lion", "prodigy"])
def test_step_without_gradients_changes_nothing(kind):
    p, grads = R.inputs(257)
    q = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = optim.Lion([q]) if kind == "lion" else optim.Prodigy([q])
    opt.step()  # before any gradient
    assert not opt.state[q] and np.array_equal(q.detach().numpy(), p)
    for g in grads[:4]:
        q.grad = torch.from_numpy(g.copy())
        opt.step()
    before = (q.detach().clone(), {k: v.clone() for k, v in opt.state[q].items()},
              {k: v for k, v in opt.param_groups[0].items() if k != "params"})
    q.grad = None
    opt.step()
    assert torch.equal(q.detach(), before[0])
    assert all(torch.equal(opt.state[q][k], v) for k, v in before[1].items())
    assert {k: v for k, v in opt.param_groups[0].items() if k != "params"} == before[2]


def test_lr_scheduler_drives_the_classes():
    """`lr` is read from the param group at every step: a torch scheduler changes what the next step uses."""
    q = torch.nn.Parameter(torch.ones(4))
    opt = optim.Lion([q], lr=1e-2)
    sched = train_util.get_lr_scheduler("cosine", opt, max_iterations=4, lr_min=1e-4)
    moved = []
    for _ in range(3):
        q.grad = torch.ones(4)
        before = q.detach().clone()
        opt.step()
        sched.step()
        moved.append(float((before - q.detach()).abs().max()))
    assert moved[0] == pytest.approx(1e-2, rel=1e-5) and moved[0] > moved[1] > moved[2] > 0


def test_get_optimizer_returns_the_classes():
    assert train_util.get_optimizer("lion") is optim.Lion and train_util.get_optimizer("Lion") is optim.Lion
    assert train_util.get_optimizer("PRODIGY") is optim.Prodigy and train_util.get_optimizer("prodigy") is optim.Prodigy
    assert train_util.get_optimizer("AdamW") is torch.optim.AdamW
    for name in ("DAdaptAdam", "AdamW8bit", "lion8bit"):
        with pytest.raises(ValueError, match="needs a package that is not installed"):
            train_util.get_optimizer(name)
    with pytest.raises(ValueError, match="Optimizer must be adam, adamw, lion or Prodigy"):
        train_util.get_optimizer("sgd")


FUSABLE = [
    ("lion", {}),
    ("Lion", {"betas": (0.95, 0.98), "weight_decay": 0.1}),
    ("lion", {"lr": 3e-5}),
    ("prodigy", {}),
    ("Prodigy", {"weight_decay": 0.01, "decouple": True, "use_bias_correction": True, "safeguard_warmup": True,
                 "d_coef": 2.0, "d0": 1e-5, "growth_rate": 1.02, "beta3": 0.99, "eps": 1e-6, "betas": (0.9, 0.99)}),
    ("PRODIGY", {"decouple": False, "weight_decay": 0.01}),
]
REFUSED = [
    ("prodigy", {"fsdp_in_use": False}, "fsdp_in_use"),
    ("prodigy", {"slice_p": 1}, "slice_p"),
    ("prodigy", {"d_coef": 2.0, "foreach": True}, "foreach"),
    ("lion", {"use_triton": False}, "use_triton"),
    ("lion", {"eps": 1e-8}, "eps"),
]


def test_optimizer_rule_table():
    for name, kwargs in FUSABLE:
        spec = TC.native_optimizer(name, kwargs)
        assert spec.name == name.lower() and "lr" not in spec.hyper
        defaults = optim.LION_DEFAULTS if spec.name == "lion" else optim.PRODIGY_DEFAULTS
        assert set(spec.hyper) == set(defaults) - {"lr"}
        assert all(spec.hyper[k] == v for k, v in kwargs.items() if k != "lr")
        assert TC.step_choice(None, name, kwargs) == (True, spec) and TC.step_choice(True, name, kwargs) == (True, spec)
        assert TC.step_choice(False, name, kwargs) == (False, None)
    for name, kwargs, arg in REFUSED:
        assert TC.native_optimizer(name, kwargs) is None
        assert TC.step_choice(None, name, kwargs) == (False, None)  # the torch class under the autograd loop
        assert TC.step_choice(False, name, kwargs) == (False, None)
        with pytest.raises(ValueError, match=arg):
            TC.step_choice(True, name, kwargs)
    # Adam / AdamW: the existing rule, unchanged, with the spec of the native AdamW beside it
    assert TC.step_choice(None, "AdamW", {}) == (True, optim.OptimSpec.adamw(weight_decay=1e-2))
    assert TC.step_choice(True, "adam", {"eps": 1e-3, "betas": (0.8, 0.9)}) == (
        True, optim.OptimSpec.adamw((0.8, 0.9), 1e-3, 0.0))
    assert TC.step_choice(None, "AdamW", {"foreach": False}) == (False, None)
    assert TC.step_choice(False, "AdamW", {}) == (False, None)
    with pytest.raises(ValueError, match="--fused_step implements Adam / AdamW"):
        TC.step_choice(True, "AdamW", {"amsgrad": True})
    with pytest.raises(ValueError):
        TC.step_choice(True, "dadaptadam", {})
    assert TC.step_choice(None, "dadaptadam", {}) == (False, None)
    # the Adam rule itself keeps what tests/test_train_common_cpu.py pins
    assert TC.adam_fusable("Lion", {})[0] is False


def test_torch_prodigy_takes_the_inert_package_arguments_only():
    q = torch.nn.Parameter(torch.ones(2))
    optim.Prodigy([q], fsdp_in_use=False, slice_p=1)
    for kw in ({"fsdp_in_use": True}, {"slice_p": 11}):
        with pytest.raises(ValueError, match="fsdp_in_use"):
            optim.Prodigy([q], **kw)


def test_native_steps_are_exported_and_documented():
    hdr = open(os.path.join(ROOT, "include", "smi.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for s in ("smi_clip_lion", "smi_prodigy_init", "smi_clip_prodigy"):
        assert s in _native.EXPORTED_SYMBOLS and f"{s}(" in hdr and s in design, s
        assert hasattr(_native.lib(), s)


def _worst_mutation_ratio(kind, mutation, n):
    fn, variants, default_lr = ((R.lion_ref, R.LION_VARIANTS, 1e-4) if kind == "lion" else
                                (R.prodigy_ref, R.PRODIGY_VARIANTS, 1.0))
    p, grads = R.inputs(n)
    worst = (0.0, None, None, None)
    for variant in variants:
        _, _, lrs, max_norm, hyper = R.reference(kind, n, variant)
        with np.errstate(invalid="ignore", divide="ignore"):  # a mutated d may turn negative
            mutated = fn(p, grads, lrs, R.F64, max_norm=max_norm, mutate=mutation, **hyper)
        ratio, q, step = R.worst_ratio(kind, n, variant, mutated)
        if ratio > worst[0]:
            worst = (ratio, variant, q, step)
    return worst


@pytest.mark.parametrize("kind,mutation", [("lion", m) for m in R.LION_MUTATIONS] +
                         [("prodigy", m) for m in R.PRODIGY_MUTATIONS])
def test_bars_see_each_mutation(kind, mutation):
    """What the bars can see: each mutated float64 restatement misses a bar by more than twice on a listed input."""
    ratio, variant, q, step = max(_worst_mutation_ratio(kind, mutation, n) for n in (257, 5000))
    print(f"{kind} {mutation}: {ratio:.3g} x the bar ({variant}, {q}, step {step})")
    assert ratio > 2.0, (ratio, variant, q, step)
