"""LPIPS v0.1 on AlexNet -- a drop-in for `lpips.LPIPS(net='alex')` in eval mode, as eval-scripts/lpip_score.py calls it:
    loss_fn_alex = lpips.LPIPS(net='alex');  l = loss_fn_alex(original, edited)          (images in [-1, 1], NCHW)
A parameter container with the `lpips` package's parameter names; the arithmetic runs in the HIP engine
(csrc/engine_lpips.hip, csrc/lpips.hip: patch-matrix, max-pool and distance-head kernels around the GEMMs).  No PyTorch
forward: without the HIP library, or on a CPU device, a call raises.

State-dict names (recalled from the `lpips` and `torchvision` packages, neither of which is installed where this was
written: DESIGN.md lists them as unpinned):
    net.slice1.0 / net.slice2.3 / net.slice3.6 / net.slice4.8 / net.slice5.10  (.weight, .bias)   the AlexNet convolutions
    lin0.model.1.weight ... lin4.model.1.weight  [1, C, 1, 1]                                     the 1x1 `lin` layers
    scaling_layer.shift / scaling_layer.scale    [1, 3, 1, 1]                                     constants of the metric
`load_state_dict` also takes torchvision's own AlexNet names (`features.{0,3,6,8,10}.*`; `classifier.*` is ignored), so
that the two released files -- torchvision's alexnet and the package's `lin` weights -- load one after the other with
strict=False, or merged with strict=True."""
from __future__ import annotations

from typing import Dict, Sequence

import torch
import torch.nn as nn

from . import _native
from .engine_cache import EngineCacheMixin

ALEX_CHANNELS = (64, 192, 384, 256, 256)
ALEX_GEOMETRY = ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))  # (kernel, stride, padding) of the five convs
FEATURE_INDEX = (0, 3, 6, 8, 10)  # position of each conv in torchvision's alexnet().features
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_SIZE = 31  # below it the second max-pool has no window


def conv_names() -> Sequence[str]:
    return [f"net.slice{i + 1}.{idx}" for i, idx in enumerate(FEATURE_INDEX)]


def canonical_state_dict(state_dict) -> Dict[str, torch.Tensor]:
    """The keys of `state_dict` under this container's names: torchvision's `features.N.*` become `net.sliceK.N.*`,
    `classifier.*` and `num_batches_tracked`-style extras of other layers are dropped, everything else is kept."""
    by_index = {f"features.{idx}.": f"{name}." for idx, name in zip(FEATURE_INDEX, conv_names())}
    out = {}
    for k, v in state_dict.items():
        if k.startswith("classifier."):
            continue
        for old, new in by_index.items():
            if k.startswith(old):
                k = new + k[len(old):]
                break
        out[k] = v
    return out


class _Indexed(nn.Module):
    """a module whose single child carries a number as its name (`slice2.3`, `model.1`), as in an nn.Sequential slice"""

    def __init__(self, index: int, child: nn.Module):
        super().__init__()
        self.add_module(str(index), child)


class _Alex(nn.Module):
    def __init__(self, channels):
        super().__init__()
        cin = 3
        for i, (idx, (k, s, p), c) in enumerate(zip(FEATURE_INDEX, ALEX_GEOMETRY, channels)):
            setattr(self, f"slice{i + 1}", _Indexed(idx, nn.Conv2d(cin, c, k, s, p)))
            cin = c


class _Lin(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.model = _Indexed(1, nn.Conv2d(c, 1, 1, bias=False))  # model.0 is the Dropout: no parameters


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1))


class LPIPS(EngineCacheMixin, nn.Module):
    _component, _handle = "LPIPS network", "lpips"

    def __init__(self, channels: Sequence[int] = ALEX_CHANNELS):
        super().__init__()
        if len(channels) != 5:
            raise ValueError(f"LPIPS: five channel widths expected, got {tuple(channels)}")
        self.channels = tuple(int(c) for c in channels)
        self.scaling_layer = _ScalingLayer()
        self.net = _Alex(self.channels)
        for i, c in enumerate(self.channels):
            setattr(self, f"lin{i}", _Lin(c))
        self._engines = {}

    @property
    def dtype(self):
        return getattr(self.lin0.model, "1").weight.dtype

    @property
    def device(self):
        return getattr(self.lin0.model, "1").weight.device

    def _apply(self, fn, *a, **kw):
        """the scaling layer's constants are fp32 scalars of the stem kernel whatever the storage type of the weights"""
        out = super()._apply(fn, *a, **kw)
        for name, vals in (("shift", SHIFT), ("scale", SCALE)):
            buf = getattr(self.scaling_layer, name)
            setattr(self.scaling_layer, name, torch.tensor(vals, dtype=torch.float32, device=buf.device).view(1, 3, 1, 1))
        return out

    def load_state_dict(self, state_dict, strict: bool = True):
        sd = canonical_state_dict(state_dict)
        for name, vals in (("scaling_layer.shift", SHIFT), ("scaling_layer.scale", SCALE)):
            if name in sd:
                got = sd[name].detach().float().flatten().cpu()
                if got.numel() != 3 or not torch.allclose(got, torch.tensor(vals), atol=1e-6):
                    raise _native.SmiError(f"LPIPS: {name} = {got.tolist()} is not the constant of LPIPS v0.1 {vals}, "
                                           f"which the stem kernel applies")
            # (the released files carry no scaling layer: its constants are part of the metric, not of a checkpoint)
            sd[name] = torch.tensor(vals, dtype=torch.float32).view(1, 3, 1, 1)
        for i in range(5):  # the lin weight as [C] or [1, C, 1, 1]
            k = f"lin{i}.model.1.weight"
            if k in sd and sd[k].ndim != 4:
                sd[k] = sd[k].reshape(1, -1, 1, 1)
        return super().load_state_dict(sd, strict=strict)

    def _new_engine(self, state, n, h, w):
        eng = {}
        for idx, name in zip(FEATURE_INDEX, conv_names()):
            eng[f"features.{idx}.weight"] = state[f"{name}.weight"].contiguous()
            eng[f"features.{idx}.bias"] = state[f"{name}.bias"].contiguous()
        for i in range(5):
            eng[f"lin{i}.weight"] = state[f"lin{i}.model.1.weight"].contiguous()
        return _native.LpipsEngine(self.channels, self.dtype, eng, max(n, 1), h, w, self.device)

    @torch.no_grad()
    def forward(self, in0, in1, normalize: bool = False):
        """in0, in1 [n, 3, H, W] in [-1, 1] (`normalize=True`: in [0, 1]) -> distances f32 [n, 1, 1, 1]"""
        if in0.ndim != 4 or in0.shape != in1.shape or in0.shape[1] != 3:
            raise _native.SmiError(f"LPIPS: two [n, 3, H, W] batches expected, got {tuple(in0.shape)} and "
                                   f"{tuple(in1.shape)}")
        if normalize:
            in0, in1 = 2 * in0.float() - 1, 2 * in1.float() - 1
        n, _, h, w = in0.shape
        dist, _, _ = self._engine(n, h, w).distance(img_a=in0, img_b=in1)
        return dist.view(n, 1, 1, 1)

    @torch.no_grad()
    def distance(self, rgb8_a, rgb8_b, want_per_layer: bool = False, want_feats: bool = False):
        """uint8 [n, H, W, 3] pairs (x = u / 127.5 - 1 on the device) -> dist f32 [n]; with a flag set, the tuple
        (dist, per_layer f32 [n, 5] or None, the five post-ReLU taps [2n, Ho, Wo, C] or None)"""
        if rgb8_a.ndim != 4 or rgb8_a.shape != rgb8_b.shape or rgb8_a.shape[-1] != 3:
            raise _native.SmiError(f"LPIPS: two uint8 [n, H, W, 3] batches expected, got {tuple(rgb8_a.shape)} and "
                                   f"{tuple(rgb8_b.shape)}")
        n, h, w, _ = rgb8_a.shape
        out = self._engine(n, h, w).distance(rgb8_a=rgb8_a, rgb8_b=rgb8_b, want_per_layer=want_per_layer,
                                              want_feats=want_feats)
        return out if (want_per_layer or want_feats) else out[0]


def init_synthetic_(model: LPIPS, seed: int) -> LPIPS:
    """Seeded weights: He-scaled filters (N sqrt(2 / fan_in)), biases 0.5 N, `lin` weights |N| / C >= 0 as the trained
    ones are; all rounded to bf16-representable values, so that fp16 and bf16 engines hold the same numbers."""
    g = torch.Generator().manual_seed(seed)
    r16 = lambda t: t.to(torch.bfloat16).to(torch.float32)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith("lin"):
                p.copy_(r16(torch.randn(p.shape, generator=g).abs() / p.shape[1]))
            elif p.ndim == 4:
                p.copy_(r16(torch.randn(p.shape, generator=g) * (2.0 / p[0].numel()) ** 0.5))
            else:
                p.copy_(r16(0.5 * torch.randn(p.shape, generator=g)))
    return model
