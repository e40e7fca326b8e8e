"""Lion and Prodigy as torch.optim.Optimizer classes of our own: the reference's get_optimizer (T/train_util.py:1014-1051)
imports them from lion_pytorch and prodigyopt, which this project does not depend on.  Plain torch, CPU and GPU tensors
alike; they serve the reference-style autograd loop (`--no_fused_step`).  The fused step runs the same algorithms as
native kernels (smi_clip_lion, smi_prodigy_init / smi_clip_prodigy; include/smi.h states both as their contract).

`lr` is read from the param group at every step, so every train_util.get_lr_scheduler applies."""
import dataclasses
import math

import torch

LION_DEFAULTS = dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0)
PRODIGY_DEFAULTS = dict(lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True,
                        use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"))


@dataclasses.dataclass(frozen=True)
class OptimSpec:
    """What the fused step needs to know of its optimiser: `name` is "adamw", "lion" or "prodigy"; `hyper` holds every
    hyper-parameter but the learning rate (the step takes that per call): the name's defaults overlaid with the
    configured keyword arguments.  AdamW: betas, eps, weight_decay."""
    name: str
    hyper: dict

    @staticmethod
    def adamw(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2) -> "OptimSpec":
        return OptimSpec("adamw", dict(betas=tuple(betas), eps=eps, weight_decay=weight_decay))

    @staticmethod
    def of(name: str, kwargs: dict) -> "OptimSpec":
        defaults = {"lion": LION_DEFAULTS, "prodigy": PRODIGY_DEFAULTS}[name]
        unknown = set(kwargs) - set(defaults)
        if unknown:
            raise ValueError(f"{name}: unknown argument(s) {sorted(unknown)}")
        hyper = {k: v for k, v in {**defaults, **kwargs}.items() if k != "lr"}
        return OptimSpec(name, hyper)


class Lion(torch.optim.Optimizer):
    """p <- p (1 - lr wd);  c = beta1 m + (1 - beta1) g;  p <- p - lr sign(c);  m <- beta2 m + (1 - beta2) g."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0):
        if lr <= 0.0 or not all(0.0 <= b <= 1.0 for b in betas):
            raise ValueError(f"Lion: lr {lr} must be positive and betas {betas} within [0, 1]")
        super().__init__(params, dict(lr=lr, betas=betas, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, (beta1, beta2), wd = group["lr"], group["betas"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if not state:
                    state["exp_avg"] = torch.zeros_like(p)
                m, g = state["exp_avg"], p.grad
                p.mul_(1.0 - lr * wd)
                c = (m * beta1).add_(g, alpha=1.0 - beta1)
                p.add_(torch.sign(c), alpha=-lr)  # sign(0) = 0: an element that never saw a gradient only decays
                m.mul_(beta2).add_(g, alpha=1.0 - beta2)
        return loss


class Prodigy(torch.optim.Optimizer):
    """Prodigy (Mishchenko & Defazio, "Prodigy: an expeditiously adaptive parameter-free learner"): Adam whose step size
    d lr is estimated on the way, d = d_coef * d_numerator / d_denom from sum g (p0 - p) and sum |s|.  One d per param
    group, the sums over all of the group's parameters; d, d_max, d_numerator and the sums are Python floats (doubles)."""

    def __init__(self, params, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True,
                 use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"),
                 fsdp_in_use=False, slice_p=1):
        if fsdp_in_use or slice_p != 1:  # the package's sharded / sub-sampled estimates: accepted only at their inert values
            raise ValueError("Prodigy: fsdp_in_use=True and slice_p != 1 are not implemented")
        if d0 <= 0.0 or lr < 0.0 or eps < 0.0 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"Prodigy: d0 {d0} > 0, lr {lr} >= 0, eps {eps} >= 0, betas {betas} within [0, 1) expected")
        super().__init__(params, dict(lr=lr, betas=betas, beta3=beta3, eps=eps, weight_decay=weight_decay,
                                      decouple=decouple, use_bias_correction=use_bias_correction,
                                      safeguard_warmup=safeguard_warmup, d0=d0, d_coef=d_coef, growth_rate=growth_rate,
                                      d=d0, d_max=d0, d_numerator=0.0, k=0))

    @property
    def d(self) -> float:
        """The current estimate of group 0 (for the progress line)."""
        return self.param_groups[0]["d"]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            live = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            lr, (beta1, beta2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            beta3 = math.sqrt(beta2) if group["beta3"] is None else group["beta3"]
            d, d0, k = group["d"], group["d0"], group["k"]
            bc = math.sqrt(1.0 - beta2 ** (k + 1)) / (1.0 - beta1 ** (k + 1)) if group["use_bias_correction"] else 1.0
            dlr = d * lr * bc
            d_numerator = beta3 * group["d_numerator"]
            d_denom = 0.0
            for p in live:
                g = p.grad
                if wd != 0 and not group["decouple"]:
                    g = g.add(p, alpha=wd)
                state = self.state[p]
                if not state:
                    state["p0"] = p.detach().clone()
                    state["s"], state["exp_avg"], state["exp_avg_sq"] = (torch.zeros_like(p) for _ in range(3))
                if lr > 0.0:
                    d_numerator += (d / d0) * dlr * torch.dot(g.flatten(), (state["p0"] - p).flatten()).item()
                state["exp_avg"].mul_(beta1).add_(g, alpha=d * (1.0 - beta1))
                state["exp_avg_sq"].mul_(beta2).addcmul_(g, g, value=d * d * (1.0 - beta2))
                state["s"].mul_(beta3).add_(g, alpha=(d / d0) * (d if group["safeguard_warmup"] else dlr))
                d_denom += state["s"].abs().sum().item()
            group["d_numerator"] = d_numerator
            if d_denom == 0:  # only zero gradients so far: the moments are updated, p, d and k are not
                continue
            if lr > 0.0:
                d_hat = group["d_coef"] * d_numerator / d_denom
                if d == d0:
                    d = max(d, d_hat)
                group["d_max"] = max(group["d_max"], d_hat)
                d = min(group["d_max"], d * group["growth_rate"])
            group["d"] = d
            for p in live:
                state = self.state[p]
                denom = state["exp_avg_sq"].sqrt().add_(d * eps)
                if wd != 0 and group["decouple"]:
                    p.add_(p, alpha=-wd * dlr)
                p.addcdiv_(state["exp_avg"], denom, value=-dlr)
            group["k"] = k + 1
        return loss
