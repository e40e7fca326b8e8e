"""Lion and Prodigy restated from the text of the specification (include/smi.h carries the same text), independently of
sliders_conceptmod_amd.optim and of the kernels: numpy only.

(A) `lion_ref` / `prodigy_ref` with `F64`: every operation in float64.
(B) the same functions with `F32`: every tensor operation rounded to fp32 the way torch's CPU kernels round it
    (x.mul_(b).add_(g, alpha=a) is fma(a, g, fl(b x)); addcmul_ is fma(fl(value g), g, x); addcdiv_ is x + fl(fl(value m) /
    denom)), sums pairwise in fp32 (numpy's), the scalars d, d_max, d_numerator and the sums in double as in (A).

The bars of the tests are 3 x dist(B, A) + 1e-12 per quantity and step (`bars`): relative L2 for vectors, relative for d.
Three is the factor of DESIGN.md section 15: room for another summation order and for fma contraction.

Inputs (`inputs`): seeded; the first gradient is all zeros (the d_denom == 0 no-op), the second meets p0 == p (d_hat = 0,
the d == d0 branch), from the third on d grows; the last two gradients turn against the earlier ones, so that d_hat falls
below d_max; a tenth of the elements carry gradients 1e-9 times the rest (d * eps decides their update); every thirteenth
element has an exactly zero gradient throughout (Lion must leave it to the decay; every lora_down at step 1)."""
import functools
import math

import numpy as np

SIZES = (1, 255, 257, 5000, 300001)  # one element; a partial and a full-plus-one workgroup; a vector tail; > 1024 workgroups
STEPS = 8
INF = float("inf")


class F64:
    dt = np.float64

    @staticmethod
    def sc(x):  # a Python scalar entering a tensor operation
        return np.float64(x)

    @staticmethod
    def fma(a, b, c):
        return a * b + c

    @staticmethod
    def sum(x):
        return float(np.sum(x))


class F32:
    dt = np.float32

    @staticmethod
    def sc(x):
        return np.float32(x)

    @staticmethod
    def fma(a, b, c):  # one rounding: the product of two fp32 numbers is exact in float64
        r = np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)
        return r.astype(np.float32)

    @staticmethod
    def sum(x):
        return float(np.sum(x, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def inputs(n: int):
    """(p, [g_1 .. g_8]) as fp32 arrays."""
    rng = np.random.default_rng(1000 + n)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    mu = rng.standard_normal(n)
    idx = np.arange(n)
    grads = []
    for t in range(STEPS):
        g = mu * (1.0 - 0.05 * t) + 0.3 * rng.standard_normal(n)
        if t >= STEPS - 2:
            g = -g
        g[idx % 10 == 3] *= 1e-9
        g[idx % 13 == 5] = 0.0
        if t == 0:
            g[:] = 0.0
        grads.append(g.astype(np.float32))
    return p, grads


def zero_gradient_elements(n: int):
    return np.arange(n) % 13 == 5


LION_VARIANTS = {
    "default": dict(),
    "decay": dict(weight_decay=0.01),
    "decay_large_lr": dict(lr=1e-2, weight_decay=0.5),  # lr^2 wd large enough for the order of decay and update to show
    "clip": dict(max_norm=0.2),
    "clip_inactive": dict(max_norm=1e6),
    "lr_schedule": dict(lrs=[1e-4 * (1.0 - 0.1 * t) for t in range(STEPS)]),
}
PRODIGY_VARIANTS = {
    "default": dict(),
    "decoupled_decay": dict(weight_decay=0.01),
    "coupled_decay": dict(weight_decay=0.01, decouple=False),
    "bias_correction": dict(use_bias_correction=True),
    "safeguard_warmup": dict(safeguard_warmup=True),
    "growth_rate_2": dict(growth_rate=2.0),
    "growth_rate_1.2": dict(growth_rate=1.2),  # below the first d_hat / d0: only the d == d0 clause lets d jump to d_hat
    "d_coef_half": dict(d_coef=0.5),
    "clip": dict(max_norm=0.2),
    "clip_inactive": dict(max_norm=1e6),
    "lr_schedule": dict(lrs=[1.0 - 0.1 * t for t in range(STEPS)]),
    "eps_large": dict(eps=0.1),  # d * eps above sqrt(exp_avg_sq) for every element: which d multiplies eps shows everywhere
}
LION_MUTATIONS = ("sign0_plus", "beta2_in_c", "decay_after_update")
PRODIGY_MUTATIONS = ("numerator_not_decayed", "new_d_in_dlr", "old_d_in_eps", "eps_unscaled", "numerator_updated_p",
                     "k_on_skipped_step", "no_d0_clause", "d_max_ignored")


def split_variant(variant: dict, default_lr: float):
    """(hyper-parameters, max_norm, per-step learning rates) of a variant entry."""
    v = dict(variant)
    max_norm = v.pop("max_norm", 0.0)
    lr = v.pop("lr", default_lr)
    lrs = v.pop("lrs", [lr] * STEPS)
    return v, max_norm, lrs


def clip(g, max_norm, ar):
    """torch.nn.utils.clip_grad_norm_(max_norm): g * min(max_norm / (|g| + 1e-6), 1)."""
    if not max_norm > 0:
        return g
    norm = np.sqrt(ar.sc(ar.sum(g * g)))
    coef = min(ar.sc(max_norm) / (norm + ar.sc(1e-6)), ar.sc(1.0))
    return g * coef


def lion_ref(p, grads, lrs, ar, betas=(0.9, 0.99), weight_decay=0.0, max_norm=0.0, mutate=None):
    """Every state vector after every step: {"p": [...], "exp_avg": [...]}."""
    beta1, beta2 = betas
    p = p.astype(ar.dt)
    m = np.zeros_like(p)
    hist = {"p": [], "exp_avg": []}
    for g, lr in zip(grads, lrs):
        g = clip(g.astype(ar.dt), max_norm, ar)
        if mutate != "decay_after_update":
            p = p * ar.sc(1.0 - lr * weight_decay)
        bc = beta2 if mutate == "beta2_in_c" else beta1
        c = ar.fma(ar.sc(1.0 - bc), g, m * ar.sc(bc))
        sgn = np.sign(c)
        if mutate == "sign0_plus":
            sgn = np.where(c >= 0, 1.0, -1.0).astype(ar.dt)
        p = ar.fma(ar.sc(-lr), sgn, p)
        if mutate == "decay_after_update":
            p = p * ar.sc(1.0 - lr * weight_decay)
        m = ar.fma(ar.sc(1.0 - beta2), g, m * ar.sc(beta2))
        hist["p"].append(p.copy())
        hist["exp_avg"].append(m.copy())
    return hist


def prodigy_ref(p, grads, lrs, ar, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True,
                use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=INF, max_norm=0.0,
                mutate=None):
    """Every state vector, d and k after every step: {"p", "exp_avg", "exp_avg_sq", "s", "d", "k"} -> lists."""
    beta1, beta2 = betas
    beta3 = math.sqrt(beta2) if beta3 is None else beta3
    p = p.astype(ar.dt)
    p0 = p.copy()
    m, v, s = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
    d = d_max = d0
    d_numerator, k = 0.0, 0
    hist = {q: [] for q in ("p", "exp_avg", "exp_avg_sq", "s", "d", "k")}

    def record():
        for q, x in (("p", p), ("exp_avg", m), ("exp_avg_sq", v), ("s", s)):
            hist[q].append(x.copy())
        hist["d"].append(d)
        hist["k"].append(k)

    for g, lr in zip(grads, lrs):
        g = clip(g.astype(ar.dt), max_norm, ar)
        bc = math.sqrt(1.0 - beta2 ** (k + 1)) / (1.0 - beta1 ** (k + 1)) if use_bias_correction else 1.0
        dlr = d * lr * bc
        if mutate != "numerator_not_decayed":
            d_numerator = beta3 * d_numerator
        if weight_decay != 0 and not decouple:
            g = ar.fma(ar.sc(weight_decay), p, g)
        m = ar.fma(ar.sc(d * (1.0 - beta1)), g, m * ar.sc(beta1))
        v = ar.fma(ar.sc(d * d * (1.0 - beta2)) * g, g, v * ar.sc(beta2))
        s = ar.fma(ar.sc((d / d0) * (d if safeguard_warmup else dlr)), g, s * ar.sc(beta3))
        if lr > 0:
            seen = p
            if mutate == "numerator_updated_p":  # the update of this step (old d throughout) applied before the product
                seen = p + (ar.sc(-dlr) * m) / (np.sqrt(v) + ar.sc(d * eps))
            d_numerator += (d / d0) * dlr * ar.sum(g * (p0 - seen))
        d_denom = ar.sum(np.abs(s))
        if d_denom == 0:
            if mutate == "k_on_skipped_step":
                k += 1
            record()
            continue
        d_old = d
        if lr > 0:
            d_hat = d_coef * d_numerator / d_denom
            if d == d0 and mutate != "no_d0_clause":
                d = max(d, d_hat)
            d_max = max(d_max, d_hat)
            d = min(d_hat if mutate == "d_max_ignored" else d_max, d * growth_rate)
        if mutate == "new_d_in_dlr":
            dlr = d * lr * bc
        d_eps = eps if mutate == "eps_unscaled" else (d_old if mutate == "old_d_in_eps" else d) * eps
        denom = np.sqrt(v) + ar.sc(d_eps)
        if weight_decay != 0 and decouple:
            p = ar.fma(ar.sc(-weight_decay * dlr), p, p)
        p = p + (ar.sc(-dlr) * m) / denom
        k += 1
        record()
    return hist


def rel(x, a) -> float:
    """Relative L2 distance of vectors, relative distance of scalars; absolute where the reference is zero."""
    x, a = np.asarray(x, np.float64), np.asarray(a, np.float64)
    den = float(np.linalg.norm(a.ravel()))
    num = float(np.linalg.norm((x - a).ravel()))
    return num / den if den > 0 else num


VECTORS = {"lion": ("p", "exp_avg"), "prodigy": ("p", "exp_avg", "exp_avg_sq", "s", "d")}


@functools.lru_cache(maxsize=None)
def reference(kind: str, n: int, variant: str):
    """(A, B, lrs, max_norm, hyper) of one case; computed once, shared by every test, never modified."""
    p, grads = inputs(n)
    if kind == "lion":
        hyper, max_norm, lrs = split_variant(LION_VARIANTS[variant], 1e-4)
        fn = lion_ref
    else:
        hyper, max_norm, lrs = split_variant(PRODIGY_VARIANTS[variant], 1.0)
        fn = prodigy_ref
    a = fn(p, grads, lrs, F64, max_norm=max_norm, **hyper)
    b = fn(p, grads, lrs, F32, max_norm=max_norm, **hyper)
    return a, b, lrs, max_norm, hyper


def bars(kind: str, n: int, variant: str):
    """{quantity: [bar after step 1, ...]} = 3 x dist(B, A) + 1e-12."""
    a, b = reference(kind, n, variant)[:2]
    return {q: [3.0 * rel(b[q][t], a[q][t]) + 1e-12 for t in range(STEPS)] for q in VECTORS[kind]}


def worst_ratio(kind: str, n: int, variant: str, got: dict):
    """max over quantities and steps of dist(got, A) / bar, with where it sits; `got` has the layout of the references."""
    a = reference(kind, n, variant)[0]
    bar = bars(kind, n, variant)
    worst = (0.0, None, None)
    for q in VECTORS[kind]:
        for t in range(STEPS):
            r = rel(got[q][t], a[q][t]) / bar[q][t]
            if r > worst[0]:
                worst = (r, q, t + 1)
    return worst
