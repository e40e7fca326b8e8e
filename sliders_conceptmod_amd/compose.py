"""Slider composition: several trained sliders on one UNet, each at its own scale, in ONE UNet pass.

The reference composes by construction -- two `LoRANetwork`s on one UNet each patch `forward` and the deltas add
(conceptmod/textsliders/lora.py:129-138).  Here the engine takes one adaptor per site, so the sliders are STACKED along the
rank axis into one adaptor: per adapted layer

    y_i = W x_i + sum_k m[i][k] (alpha_k / r_k) up_k(down_k(x_i))          (sample i, slider k)

is the rank-R delta (R = sum_k r_k) of down = [down_1; ...; down_K], up = [c_1 up_1 | ... | c_K up_K], with the columns of
xa = x down^T multiplied by m[i][slider of the column].  `SliderStack` plans the stacked site list (the union of the sliders'
sites in `LoRANetwork` order; the block of a slider that does not adapt a site is zeros, so a fused q|k|v group is adapted
as a whole), owns the stacked flat fp32 buffers, fills them with one `smi_lora_stack` launch and registers itself as
`unet._lora_network`.  Two routes:

  table  Linear-only stacks keep c_k = alpha_k / r_k folded into `up` and send the scales as a multiplier per (sample,
         slider) through `smi_unet_forward_compose`: a whole grid of scales is one batched pass.
  fold   stacks with conv sites (c3lier) fold c_k = s_k alpha_k / r_k and run the plain batched forward at multiplier 1 (one
         re-stack launch whenever the scales change); the engine has no per-sample multipliers on conv sites, so a grid with
         unequal rows is refused.

Refused, with a ValueError that names the cause: DoRA files (the DoRA delta is not additive in rank), files whose layers
match no train method of this UNet, and any use under `torch.enable_grad()` with an input that requires a gradient
(training or differentiating through a stack is out of scope; the stack's own buffers never require one).
`LoRANetwork` is unchanged: a second `LoRANetwork` on the same UNet still replaces the first.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from . import _native
from . import lora as LM


TABLE_FLOATS = 3072  # csrc/engine.h COL_TABLE_FLOATS: n_adapted x sum(ranks) of one smi_unet_forward_compose


@dataclass
class SliderParams:
    """One slider of a stack: what `generate_images.lora_file_params` reads from its state dict."""
    name: str
    rank: int
    alpha: float
    train_method: str
    target_replace: list
    state: Dict[str, torch.Tensor]

    @property
    def lora_names(self):
        return {k[:-len(".lora_down.weight")] for k in self.state if k.endswith(".lora_down.weight")}


@dataclass
class StackSite:
    lora_name: str
    target_path: str
    is_conv: bool
    row_len: int            # floats per lora_down row: `in` (Linear), Cin * kh * kw (conv)
    n_out: int              # rows of lora_up
    ranks: List[int]        # r_k(site): the slider's rank here (conv sites clamp it to min(rank, Cin, Cout))
    present: List[bool]     # whether slider k adapts this site (else its block is zeros)
    c0: List[int]           # first rank column of slider k
    off_down: int = 0
    off_up: int = 0

    @property
    def rank(self) -> int:
        return sum(self.ranks)


@dataclass
class StackPlan:
    sites: List[StackSite] = field(default_factory=list)
    n_down: int = 0
    n_up: int = 0

    @property
    def has_conv(self) -> bool:
        return any(s.is_conv for s in self.sites)


def slider_params(unet, slider, name: Optional[str] = None) -> SliderParams:
    """`slider`: a LoRA file (.pt / .safetensors), a state dict, or a LoRANetwork built on another UNet object of the same
    architecture."""
    from .generate_images import load_lora_state, lora_file_params
    if isinstance(slider, (str, os.PathLike)):
        name = name or os.path.splitext(os.path.basename(str(slider)))[0]
        state = load_lora_state(str(slider))
    elif isinstance(slider, LM.LoRANetwork):
        state = slider.state_dict()
    elif isinstance(slider, dict):
        state = slider
    else:
        raise TypeError(f"a slider is a LoRA file, a state dict or a LoRANetwork, not {type(slider).__name__}")
    name = name or "slider"
    if any(k.endswith("dora_scale") for k in state):
        raise ValueError(f"slider '{name}' is a DoRA file (it has dora_scale entries): the DoRA delta renormalises the "
                         f"whole weight and is not additive in rank, so it cannot be stacked")
    if torch.is_grad_enabled() and any(isinstance(v, torch.Tensor) and v.requires_grad for v in state.values()):
        raise ValueError(f"slider '{name}': its tensors require a gradient under torch.enable_grad(); training through a "
                         f"stack is out of scope (detach them, or build the stack under torch.no_grad())")
    try:
        rank, alpha, method, target_replace = lora_file_params(state, unet)
    except ValueError as e:
        raise ValueError(f"slider '{name}': {e}") from e
    return SliderParams(name, rank, alpha, method, target_replace, state)


def plan_stack(unet, sliders: Sequence[SliderParams]) -> StackPlan:
    """The stacked site list: the union of the sliders' sites in LoRANetwork order (the name / class-name walk of
    lora.select_targets), every site with rank sum_k r_k(site), `down` blocks then `up` blocks laid out site after site --
    the projections fused into one GEMM (to_q, to_k, to_v) stay adjacent with equal rank, as the engine asks."""
    names = [p.lora_names for p in sliders]
    union = set().union(*names) if names else set()
    plan = StackPlan()
    od = ou = 0
    every = LM.UNET_TARGET_REPLACE_MODULE_TRANSFORMER + LM.UNET_TARGET_REPLACE_MODULE_CONV
    for lora_name, path, child in LM.select_targets(unet, "full", every, LM.LORA_PREFIX_UNET, "_"):
        if lora_name not in union:
            continue
        ranks, c0, c = [], [], 0
        for p in sliders:
            r, dshape, ushape = LM.lora_shapes(child, p.rank)
            ranks.append(r)
            c0.append(c)
            c += r
        row_len = 1
        for d in dshape[1:]:
            row_len *= d
        site = StackSite(lora_name, path, isinstance(child, nn.Conv2d), row_len, ushape[0], ranks,
                         [lora_name in n for n in names], c0, od, ou)
        for p, r, here in zip(sliders, ranks, site.present):
            if here:
                d, u = p.state[f"{lora_name}.lora_down.weight"], p.state[f"{lora_name}.lora_up.weight"]
                if d.numel() != r * row_len or u.numel() != site.n_out * r:
                    raise ValueError(f"slider '{p.name}': {lora_name} has shapes {tuple(d.shape)} / {tuple(u.shape)}, "
                                     f"not rank {r} on a [{site.n_out}, {row_len}] layer of this UNet")
        plan.sites.append(site)
        od += site.rank * row_len
        ou += site.n_out * site.rank
    plan.n_down, plan.n_up = od, ou
    return plan


def site_coefs(sliders: Sequence[SliderParams], site: StackSite, scales: Optional[Sequence[float]] = None) -> List[float]:
    """c_k of a site: alpha_k / r_k(site) (LoRAModule.scale; the CLAMPED rank divides, lora.py:118-119), times s_k when folded.
    One fp32 product either way, as the stack kernel's single multiply expects."""
    out = []
    for k, p in enumerate(sliders):
        c = torch.tensor(p.alpha / site.ranks[k], dtype=torch.float32)
        if scales is not None:
            c = torch.tensor(float(scales[k]), dtype=torch.float32) * c
        out.append(float(c))
    return out


def grid_multiplier_rows(scale_rows: Sequence[Sequence[float]], num_samples: int) -> List[List[float]]:
    """Multiplier rows of one batched CFG pass over `scale_rows` cells: the batch is [uncond of every cell ; cond of every
    cell], `num_samples` samples per cell, and BOTH halves are adapted (as in the reference, whose patched forwards see the
    whole CFG batch)."""
    half = [[float(s) for s in row] for row in scale_rows for _ in range(num_samples)]
    return half + [list(r) for r in half]


class SliderStack:
    """K sliders on one UNet.  `set_scales([s_1..s_K])`: one scale per slider for every sample; `set_scale_grid(rows)`: one
    row of K scales per adapted sample of the next passes; `with stack:` switches the adaptor on, leaving switches it off
    (as LoRANetwork does).  Inference only."""

    def __init__(self, unet, sliders: Sequence):
        if not sliders:
            raise ValueError("a stack needs at least one slider")
        self.sliders = [slider_params(unet, s, None if isinstance(s, (str, os.PathLike)) else f"slider {i}")
                        for i, s in enumerate(sliders)]
        self.plan = plan_stack(unet, self.sliders)
        if not self.plan.sites:
            raise ValueError("the sliders adapt no layer of this UNet")
        self.ranks = [p.rank for p in self.sliders]
        self.fold = self.plan.has_conv  # conv sites: scales folded into up, no per-sample table
        dev = unet.device
        self.flat = torch.zeros(max(self.plan.n_down + self.plan.n_up, 1), dtype=torch.float32, device=dev)
        self._src = [{k: v.detach().to(dev, torch.float32).contiguous() for k, v in p.state.items()
                      if k.endswith(".weight")} for p in self.sliders]
        self._scales = [1.0] * len(self.sliders)
        self._grid: Optional[List[List[float]]] = None
        self._on = False
        self._stacked_for = None  # the scales folded into `flat` (fold route) / () once filled (table route)
        self._jobs_dev = None
        if dev.type == "cuda":
            self._restack()
        unet.__dict__["_lora_network"] = self  # as LoRANetwork: a plain attribute, not a child module

    # ---- stacked buffers ---------------------------------------------------------------------------------------
    @property
    def flat_down(self) -> torch.Tensor:
        return self.flat[:self.plan.n_down]

    @property
    def flat_up(self) -> torch.Tensor:
        return self.flat[self.plan.n_down:self.plan.n_down + self.plan.n_up]

    def stack_jobs(self):
        """The job table of smi_lora_stack, one job per (site, slider)."""
        jobs = (_native.LoraStackJobC * (len(self.plan.sites) * len(self.sliders)))()
        esz = 4
        down0, up0 = self.flat_down.data_ptr(), self.flat_up.data_ptr()
        i = 0
        for site in self.plan.sites:
            coefs = site_coefs(self.sliders, site, self._scales if self.fold else None)
            for k in range(len(self.sliders)):
                j = jobs[i]
                i += 1
                if site.present[k]:
                    j.src_down = self._src[k][f"{site.lora_name}.lora_down.weight"].data_ptr()
                    j.src_up = self._src[k][f"{site.lora_name}.lora_up.weight"].data_ptr()
                else:
                    j.src_down = j.src_up = None
                j.dst_down = down0 + site.off_down * esz
                j.dst_up = up0 + site.off_up * esz
                j.row_len, j.r, j.c0, j.R, j.n_out = site.row_len, site.ranks[k], site.c0[k], site.rank, site.n_out
                j.coef = coefs[k]
        return jobs

    def _restack(self):
        want = tuple(self._scales) if self.fold else ()
        if self._stacked_for == want:
            return
        if self.flat.device.type != "cuda":
            raise _native.SmiError("the stacked buffers are built on an MI355X by the HIP library; build the stack on a UNet "
                                   "that lives on a cuda device (there is no CPU fallback)")
        jobs = self.stack_jobs()
        if self._jobs_dev is None:
            self._jobs_dev = torch.empty(C.sizeof(jobs), dtype=torch.uint8, device=self.flat.device)
        with torch.cuda.device(self.flat.device):
            _native.check(_native.lib().smi_lora_stack(jobs, len(jobs), _native.ptr(self._jobs_dev), _native.stream_ptr()),
                          "smi_lora_stack")
        self._stacked_for = want

    # ---- scales ----------------------------------------------------------------------------------------------------
    def set_scales(self, scales: Sequence[float]):
        if len(scales) != len(self.sliders):
            raise ValueError(f"{len(scales)} scales for {len(self.sliders)} sliders")
        self._scales = [float(s) for s in scales]
        self._grid = None

    def set_scale_grid(self, rows: Sequence[Sequence[float]]):
        rows = [[float(s) for s in r] for r in rows]
        if not rows or any(len(r) != len(self.sliders) for r in rows):
            raise ValueError(f"a scale grid is a list of rows of {len(self.sliders)} scales, one row per adapted sample")
        if self.fold:
            if any(r != rows[0] for r in rows):
                raise ValueError("this stack has conv (c3lier) sites: their scales are folded into lora_up and the engine has "
                                 "no per-sample multipliers on conv sites, so every row of the grid must be equal -- run "
                                 "cells of different scales in separate passes")
            self.set_scales(rows[0])
            return
        self._grid = rows

    def scale_state(self):
        """What set_scales / set_scale_grid last set, for `restore_scale_state` (slider_grid_latents puts it back)."""
        return list(self._scales), None if self._grid is None else [list(r) for r in self._grid]

    def restore_scale_state(self, state):
        self._scales, self._grid = list(state[0]), state[1]

    @property
    def max_samples(self) -> int:
        """Samples one table-route pass can take: the engine's multiplier table holds TABLE_FLOATS entries, sum(ranks) per
        sample (smi_unet_forward_compose refuses more)."""
        return TABLE_FLOATS // sum(self.ranks)

    def __enter__(self):
        self._on = True

    def __exit__(self, exc_type, exc_value, tb):
        self._on = False

    # ---- what unet.py needs from a network -------------------------------------------------------------------------
    def engine_sites(self):
        return [{"target": s.target_path, "off_down": s.off_down, "off_up": s.off_up, "rank": s.rank, "scale": 1.0}
                for s in self.plan.sites]

    def engine_params(self):
        """(flat buffer, number of lora_down elements, multiplier): 1 while the stack is on -- its scales live in `up`
        (fold route) or in the column table (table route, `engine_compose`) -- else 0."""
        if self._on:
            self._restack()
        return self.flat, self.plan.n_down, 1.0 if self._on else 0.0

    def check_inference(self, *inputs):
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in inputs):
            raise ValueError("a SliderStack is inference only: an input requires a gradient under torch.enable_grad(); "
                             "training or differentiating through a stack is out of scope (use torch.no_grad())")

    def engine_compose(self, n: int):
        """(ranks, n multiplier rows) for a pass over n samples while a table-route stack is on, else None."""
        if not self._on or self.fold:
            return None
        if self._grid is None:
            return self.ranks, [list(self._scales) for _ in range(n)]
        if len(self._grid) != n:
            raise ValueError(f"the scale grid has {len(self._grid)} rows but the UNet batch has {n} samples")
        return self.ranks, self._grid
