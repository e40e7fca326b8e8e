"""The tail backward's export: declared in include/smi.h, bound in _native with the header's arity, present in the built
library, and routed by the step classes only at guidance scale exactly 1 (host-side checks, no GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_backward_is_declared_bound_and_exported():
    from sliders_conceptmod_amd import _native
    header = open(os.path.join(ROOT, "include", "smi.h")).read()
    m = re.search(r"int\s+smi_unet_backward_tail\s*\(([^;]*)\)\s*;", header)
    assert m, "smi_unet_backward_tail is not declared in include/smi.h"
    n_params = len([a for a in m.group(1).split(",") if a.strip()])
    assert "smi_unet_backward_tail" in _native.EXPORTED_SYMBOLS
    res, args = _native._SIGS["smi_unet_backward_tail"]
    assert res is ctypes.c_int and len(args) == n_params == 5
    assert args[1] is ctypes.c_int  # n_live
    from sliders_conceptmod_amd import build as smi_build
    lib = ctypes.CDLL(smi_build.build())
    assert hasattr(lib, "smi_unet_backward_tail") and hasattr(lib, "smi_unet_backward")


def test_tail_backward_routing_rule(monkeypatch):
    from sliders_conceptmod_amd.step import tail_backward_ok
    monkeypatch.delenv("SMI_FULL_BACKWARD", raising=False)
    assert tail_backward_ok(1.0) and tail_backward_ok(1)
    assert not tail_backward_ok(3.0) and not tail_backward_ok(0.0) and not tail_backward_ok(1.0 + 1e-6)
    assert not tail_backward_ok(1.0, allowed=False)
    monkeypatch.setenv("SMI_FULL_BACKWARD", "1")
    assert not tail_backward_ok(1.0)
