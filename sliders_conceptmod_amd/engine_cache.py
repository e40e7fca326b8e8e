"""What the `nn.Module` containers of the forward-only engines (`AutoencoderKL`, `AutoencoderKLDecoder`,
`CLIPTextModel`) share: the guard that refuses a CPU device or a dtype the engines do not have, a cache of engines keyed
on dtype, device and shape, and the rule for when that cache is stale.

An engine copies some weights into its workspace at creation (conv filters, fused q|k|v) and keeps raw pointers to the
rest (biases, norm scales, plain linear weights), so it is valid only for the parameter storage and values it was created
from.  Whatever replaces or moves the parameters -- `load_state_dict`, `.to()`, `.half()`, ... -- therefore closes every
engine; the next call builds a new one.  (Writing into a parameter in place is not seen: call `_close_engines()`.)"""
from __future__ import annotations

from . import _native


class EngineCacheMixin:
    """Goes in front of nn.Module in the bases.  The container sets `_component` / `_handle` (its names in the guard's
    message), `self._engines = {}` in __init__, has `dtype` / `device`, and builds an engine in `_new_engine`."""

    _component = ""  # "VAE encoder"
    _handle = ""     # "vae": how callers name the object they would move to the GPU

    def _new_engine(self, state: dict, n: int, *shape):
        raise NotImplementedError

    def _engine(self, n: int, *shape):
        """The engine for `shape` (h, w for the VAEs, nothing for CLIP) that takes a batch of n: cached, or (re)created."""
        if self.device.type != "cuda":
            raise _native.SmiError(f"the {self._component} runs only on an MI355X through the HIP engine; move it to a "
                                   f"cuda device with {self._handle}.to(device, dtype) (there is no CPU fallback)")
        if self.dtype not in _native.DTYPE_CODE:
            raise _native.SmiError(f"engine dtypes are float16/bfloat16, got {self.dtype}")
        key = (self.dtype, str(self.device)) + shape
        e = self._engines.get(key)
        if e is None or e.batch < n:
            if e is not None:
                e.close()
            state = {k: v.detach() for k, v in self.state_dict().items()}
            e = self._engines[key] = self._new_engine(state, n, *shape)
        return e

    def _close_engines(self):
        for e in self._engines.values():
            e.close()
        self._engines = {}

    def _apply(self, fn, *a, **kw):
        self._close_engines()
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, state_dict, *a, **kw):
        self._close_engines()
        return super().load_state_dict(state_dict, *a, **kw)
