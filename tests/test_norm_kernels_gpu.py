"""GroupNorm and LayerNorm of csrc/norm.hip, every launch form the engine uses, one launch at a time on a real MI355X through
the test entries (include/smi.h smi_op_groupnorm_ex / smi_op_layernorm_ex), against the float64 references of
tests/norm_refs.py on the same 16-bit-rounded inputs.

Every case asserts
  * what ran (one launch / two launches / two launches + fold, chunk and slot count; LayerNorm's vectors per lane and rows
    per wave) equals the restated dispatcher of norm_refs;
  * every element of y and dx within SLACK * E of the float64 reference, E the per-element bounds of norm_refs
    (test_norm_refs_cpu.py shows on these inputs that a correct fp32 kernel stays inside 1.0 E and each listed fault leaves
    SLACK * E);
  * the saved statistics within the bar |rstd / rstd64 - 1| <= 2^-14, |mean - mean64| rstd64 <= 2^-14, and a, b (GroupNorm)
    equal to rstd gamma and beta - mean a formed from the saved fp32 statistics, within 4 fp32 roundings;
  * outputs are NaN-prefilled and the NaN guard rows on both sides of y, dx and the scratch are untouched.
The worst ratios per kernel form, output and dtype are printed when the module ends (DESIGN.md holds the table);
SMI_NORM_RATIO_JSON=<path> also writes them to a file."""
import ctypes as C
import json
import os

import pytest
import torch

import norm_refs as R

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
DT_IDS = ["f16", "bf16"]
_RATIOS = {}


@pytest.fixture(scope="module")
def lib():
    from sliders_conceptmod_amd import _native
    assert torch.cuda.is_available(), "these tests need the GPU box"
    yield _native.lib()
    rows = [{"form": f, "output": o, "dtype": d, "max_ratio": round(r, 3)} for (f, o, d), r in sorted(_RATIOS.items())]
    for r in rows:
        print(f"norm max ratio to bound  {r['form']:22s} {r['output']:5s} {r['dtype']:5s} {r['max_ratio']:.3f}")
    if os.environ.get("SMI_NORM_RATIO_JSON"):
        with open(os.environ["SMI_NORM_RATIO_JSON"], "w") as f:
            json.dump(rows, f, indent=1)


def sync_or_stop():
    """A GPU error is sticky: nothing more is started on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, session stopped: {e}", returncode=3)


def dname(dt):
    return "f16" if dt == torch.float16 else "bf16"


def note(form, out, dt, ratio):
    k = (form, out, dname(dt))
    _RATIOS[k] = max(_RATIOS.get(k, 0.0), ratio)


def err(lib):
    m = lib.smi_last_error()
    return m.decode() if m else ""


def ran_tuple(r, ln=False):
    return (r.form, r.nv, r.r) if ln else (r.form, r.chunks, r.slots)


def run_gn(lib, case, inp, dt, sel=-1, silu=None, stats_only=False, bwd=True, add=None, n0=0, expect_rc0=True):
    """One smi_op_groupnorm_ex call on guarded, NaN-prefilled buffers.  add: None, "sep" or "alias".  Returns a dict."""
    from sliders_conceptmod_amd._native import NormArgsC, NormRanC
    nb, HW, Cc, G = case.nb, case.HW, case.C, case.G
    silu = case.silu if silu is None else silu
    y = R.Guarded(nb * HW, Cc, dt, "cuda")
    dx = R.Guarded((nb - n0) * HW, Cc, dt, "cuda")
    scr = R.Guarded(R.gn_scratch_floats(nb, HW, Cc, G), 1, torch.float32, "cuda", g=64)
    dy = inp["dy"][n0:].contiguous()
    ad = inp["add"][n0:].contiguous()
    a = NormArgsC()
    a.x, a.gamma, a.beta = inp["x"].data_ptr(), inp["gamma"].data_ptr(), inp["beta"].data_ptr()
    a.y = None if stats_only else y.view.data_ptr()
    if bwd:
        a.dy, a.dx = dy.data_ptr(), dx.view.data_ptr()
        if add == "sep":
            a.add = ad.data_ptr()
        elif add == "alias":
            dx.view.copy_(ad.reshape(-1, Cc))
            a.add = dx.view.data_ptr()
    a.scratch = scr.view.data_ptr()
    a.dtype = 0 if dt == torch.float16 else 1
    a.nb, a.hw, a.c, a.g, a.eps, a.silu, a.bwd_n0, a.sel_fused = nb, HW, Cc, G, case.eps, silu, n0, sel
    rf, rb = NormRanC(), NormRanC()
    rc = lib.smi_op_groupnorm_ex(C.byref(a), C.byref(rf), C.byref(rb))
    sync_or_stop()
    if expect_rc0:
        assert rc == 0, err(lib)
    s = scr.view[:, 0]
    return dict(rc=rc, y=y.view.reshape(nb, HW, Cc), dx=dx.view.reshape(nb - n0, HW, Cc), a=s[:nb * Cc].reshape(nb, Cc),
                b=s[nb * Cc:2 * nb * Cc].reshape(nb, Cc), mr=s[2 * nb * Cc:2 * nb * Cc + nb * G * 2].reshape(nb, G, 2),
                ran_fwd=ran_tuple(rf), ran_bwd=ran_tuple(rb), bufs=(y, dx, scr), dy=dy, add=ad)


def cuda_inputs(case, dt, ln=False):
    inp = R.ln_inputs(case, dt) if ln else R.gn_inputs(case, dt)
    return {k: v.cuda() for k, v in inp.items()}


def check_gn(case, inp, dt, out, silu, add, n0, form_name, what=("y", "dx", "stats")):
    """E per element, the statistics bar, a and b against the saved statistics."""
    dy, ad = out["dy"], (out["add"] if add else None)
    ref = R.gn_ref(inp["x"], inp["gamma"], inp["beta"], case.G, case.eps, silu, dy, ad, n0=n0)
    E_y, E_dx = R.gn_bounds(ref, inp["x"], inp["gamma"], inp["beta"], case.G, silu, dt, dy, ad, n0=n0)
    cpg = case.C // case.G
    if "y" in what:
        r = R.worst(out["y"], ref["y"], E_y)
        note(form_name, "y", dt, r)
        print(f"{case.name} {dname(dt)} {form_name} silu={silu}: y at {r:.3f} E")
        assert r <= R.SLACK, f"{case.name}: y at {r:.3f} E ({form_name})"
    if "stats" in what:
        mean, rstd = out["mr"][..., 0], out["mr"][..., 1]
        sr, sm = R.stat_worst(mean, rstd, ref)
        note(form_name, "rstd", dt, sr)
        note(form_name, "mean", dt, sm)
        print(f"{case.name} {dname(dt)} {form_name}: rstd at {sr:.3f}, mean at {sm:.3f} of the bar")
        assert sr <= 1.0 and sm <= 1.0, f"{case.name}: rstd at {sr:.3f}, mean at {sm:.3f} of the bar ({form_name})"
        # a = rstd gamma, b = beta - mean a, from the SAVED statistics: two and three fp32 roundings
        a64 = rstd.double().repeat_interleave(cpg, 1) * inp["gamma"].double()
        b64 = inp["beta"].double() - mean.double().repeat_interleave(cpg, 1) * a64
        ea = (out["a"].double() - a64).abs() / (2 * R.U32 * a64.abs() + R.FLOOR)
        eb = (out["b"].double() - b64).abs() / (4 * R.U32 * ((mean.double().repeat_interleave(cpg, 1) * a64).abs() + b64.abs()) + R.FLOOR)
        assert float(ea.max()) <= 1.0 and float(eb.max()) <= 1.0, f"{case.name}: a at {float(ea.max()):.2f}, b at {float(eb.max()):.2f} of their fp32 bound"
    if "dx" in what:
        if case.data == "const":
            E_dx[:, :, :cpg] = float("inf")  # the constant group: finite is all that is asked
        r = R.worst(out["dx"], ref["dx"], E_dx)
        note("backward", "dx", dt, r)
        print(f"{case.name} {dname(dt)} silu={silu} add={add} n0={n0}: dx at {r:.3f} E")
        assert r <= R.SLACK, f"{case.name}: dx at {r:.3f} E (silu={silu}, add={add}, n0={n0})"
    for b in out["bufs"]:
        assert b.guards_intact(), f"{case.name}: a guard row was written"


FORMS = {R.GN_ONE: "one launch", R.GN_TWO: "two launches", R.GN_FOLD: "two launches + fold"}


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("name", [c.name for c in R.GN_GEOMETRY])
def test_groupnorm_geometry(lib, name, dt):
    """Every (C, G) and HW: forward in each form the shape can take, backward with and without SiLU, add absent / separate /
    aliased, on the sub-ranges [1, 3) and [2, 3) of the batch, and the statistics-only launch."""
    case = R.GN_CASES[name]
    inp = cuda_inputs(case, dt)
    HW, Cc, G = case.HW, case.C, case.G
    sels = [-1, 0] if R.gn_fused_ok(HW, Cc, G) else [-1]
    for silu in (1, 0):
        full = None
        for sel in sels:
            o = run_gn(lib, case, inp, dt, sel=sel, silu=silu, add="sep")
            assert o["ran_fwd"] == R.gn_expected_ran(HW, Cc, G, sel), (o["ran_fwd"], sel)
            assert o["ran_bwd"] == R.gn_expected_ran(HW, Cc, G, sel, "bwd"), o["ran_bwd"]
            check_gn(case, inp, dt, o, silu, True, 0, FORMS[o["ran_fwd"][0]])
            full = o
        # `full` came from the two-launch forward (sel 0 where the one-launch form exists): the variants below use that one too
        sel = sels[-1]
        plain = run_gn(lib, case, inp, dt, sel=sel, silu=silu, add=None)
        check_gn(case, inp, dt, plain, silu, False, 0, FORMS[plain["ran_fwd"][0]], what=("dx",))
        alias = run_gn(lib, case, inp, dt, sel=sel, silu=silu, add="alias")
        assert torch.equal(alias["dx"].view(torch.int16), full["dx"].view(torch.int16)), "add aliased to dx differs from add apart"
        for n0 in (1, case.nb - 1):
            sub = run_gn(lib, case, inp, dt, sel=sel, silu=silu, add="sep", n0=n0)
            assert torch.equal(sub["dx"].view(torch.int16), full["dx"][n0:].view(torch.int16)), f"backward on samples [{n0}, nb) differs"
            assert sub["bufs"][1].guards_intact()
    # statistics only: bit-equal to the two-launch forward's a, b and mean_rstd, y never touched
    two = run_gn(lib, case, inp, dt, sel=0, bwd=False)
    st = run_gn(lib, case, inp, dt, sel=-1, stats_only=True, bwd=False)
    assert st["ran_fwd"] == R.gn_expected_ran(HW, Cc, G, 0, "stats")
    for k in ("a", "b", "mr"):
        assert torch.equal(st[k].view(torch.int32), two[k].view(torch.int32)), f"statistics-only {k} differs from the two-launch forward"
    assert st["bufs"][0].untouched() and st["bufs"][1].untouched() and st["bufs"][2].guards_intact()
    assert two["bufs"][1].untouched()


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("name", [c.name for c in R.GN_NUMERICS])
def test_groupnorm_numerics(lib, name, dt):
    """Offsets up to |mean| / std = 256, tiny and zero variance, large values, a loss-scaled gradient, saturated SiLU and an
    outlier row at each chunk edge: in every forward form the shape can take."""
    case = R.GN_CASES[name]
    inp = cuda_inputs(case, dt)
    sels = [-1, 0] if R.gn_fused_ok(case.HW, case.C, case.G) else [-1]
    for sel in sels:
        o = run_gn(lib, case, inp, dt, sel=sel, add="sep")
        assert o["ran_fwd"] == R.gn_expected_ran(case.HW, case.C, case.G, sel)
        check_gn(case, inp, dt, o, case.silu, True, 0, FORMS[o["ran_fwd"][0]])
        assert torch.isfinite(o["dx"].float()).all() and torch.isfinite(o["y"].float()).all()
    if case.HW == 1024:  # the one-launch form on a map it is not tuned for, where its slice is 20 KB
        o = run_gn(lib, case, inp, dt, sel=1, bwd=False)
        assert o["ran_fwd"] == (R.GN_ONE, 0, 0)
        check_gn(case, inp, dt, o, case.silu, False, 0, "one launch", what=("y", "stats"))


def run_ln(lib, case, inp, dt, bwd=True, add=None, row0=0, expect_rc0=True):
    from sliders_conceptmod_amd._native import NormArgsC, NormRanC
    M, Cc = case.M, case.C
    y = R.Guarded(M, Cc, dt, "cuda")
    dx = R.Guarded(M - row0, Cc, dt, "cuda")
    mr = R.Guarded(M, 2, torch.float32, "cuda", g=8)
    dy, ad = inp["dy"][row0:].contiguous(), inp["add"][row0:].contiguous()
    a = NormArgsC()
    a.x, a.gamma, a.beta, a.y = inp["x"].data_ptr(), inp["gamma"].data_ptr(), inp["beta"].data_ptr(), y.view.data_ptr()
    if bwd:
        a.dy, a.dx = dy.data_ptr(), dx.view.data_ptr()
        if add == "sep":
            a.add = ad.data_ptr()
        elif add == "alias":
            dx.view.copy_(ad)
            a.add = dx.view.data_ptr()
    a.scratch = mr.view.data_ptr()
    a.dtype = 0 if dt == torch.float16 else 1
    a.nb, a.c, a.eps, a.bwd_n0, a.sel_fused = M, Cc, R.EPS, row0, -1
    rf, rb = NormRanC(), NormRanC()
    rc = lib.smi_op_layernorm_ex(C.byref(a), C.byref(rf), C.byref(rb))
    sync_or_stop()
    if expect_rc0:
        assert rc == 0, err(lib)
    return dict(rc=rc, y=y.view, dx=dx.view, mr=mr.view, ran_fwd=ran_tuple(rf, True), ran_bwd=ran_tuple(rb, True),
                bufs=(y, dx, mr), dy=dy, add=ad)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("name", [c.name for c in R.LN_CASES_LIST])
def test_layernorm(lib, name, dt):
    case = R.LN_CASES[name]
    inp = cuda_inputs(case, dt, ln=True)
    M, Cc = case.M, case.C
    o = run_ln(lib, case, inp, dt, add="sep")
    assert o["ran_fwd"] == R.ln_expected_ran(M, Cc, False) and o["ran_bwd"] == R.ln_expected_ran(M, Cc, True), (o["ran_fwd"], o["ran_bwd"])
    ref = R.ln_ref(inp["x"], inp["gamma"], inp["beta"], R.EPS, o["dy"], o["add"])
    E_y, E_dx = R.ln_bounds(ref, inp["x"], inp["gamma"], inp["beta"], dt, o["dy"], o["add"])
    ry, rdx = R.worst(o["y"], ref["y"], E_y), R.worst(o["dx"], ref["dx"], E_dx)
    sr, sm = R.stat_worst(o["mr"][:, 0], o["mr"][:, 1], ref)
    form = f"layernorm nv{o['ran_fwd'][1]} r{o['ran_fwd'][2]}"
    for k, v in (("y", ry), ("dx", rdx), ("rstd", sr), ("mean", sm)):
        note(form, k, dt, v)
    print(f"{name} {dname(dt)}: y {ry:.3f} E, dx {rdx:.3f} E, rstd {sr:.3f}, mean {sm:.3f} of the bar")
    assert ry <= R.SLACK and rdx <= R.SLACK, (ry, rdx)
    assert sr <= 1.0 and sm <= 1.0, (sr, sm)
    plain = run_ln(lib, case, inp, dt, add=None)
    refp = R.ln_ref(inp["x"], inp["gamma"], inp["beta"], R.EPS, plain["dy"], None)
    _, E_p = R.ln_bounds(refp, inp["x"], inp["gamma"], inp["beta"], dt, plain["dy"], None)
    assert R.worst(plain["dx"], refp["dx"], E_p) <= R.SLACK
    alias = run_ln(lib, case, inp, dt, add="alias")
    assert torch.equal(alias["dx"].view(torch.int16), o["dx"].view(torch.int16)), "add aliased to dx differs from add apart"
    if M > 3:
        sub = run_ln(lib, case, inp, dt, add="sep", row0=3)
        assert torch.equal(sub["dx"].view(torch.int16), o["dx"][3:].view(torch.int16)), "backward on rows [3, M) differs"
        assert sub["bufs"][1].guards_intact()
    for out in (o, plain, alias):
        for b in out["bufs"]:
            assert b.guards_intact(), f"{name}: a guard row was written"


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("Cc,G,word", [(12, 4, "multiple of 8"), (64, 3, "multiple of 8 and of G"), (8200, 25, "LDS")])
def test_groupnorm_refusals(lib, dt, Cc, G, word):
    case = R.GnCase("refused", 4, Cc, G, nb=1)
    inp = {k: torch.zeros(s, dtype=dt, device="cuda") for k, s in
           dict(x=(1, 4, Cc), dy=(1, 4, Cc), add=(1, 4, Cc), gamma=(Cc,), beta=(Cc,)).items()}
    for stats_only in (False, True):
        o = run_gn(lib, case, inp, dt, stats_only=stats_only, expect_rc0=False)
        assert o["rc"] < 0 and word in err(lib), (o["rc"], err(lib))
        assert o["ran_fwd"] == (0, 0, 0)
        assert all(b.untouched() for b in o["bufs"])


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("Cc", [12, 2056])
def test_layernorm_refusals(lib, dt, Cc):
    case = R.LnCase("refused", 3, Cc)
    inp = {k: torch.zeros(s, dtype=dt, device="cuda") for k, s in
           dict(x=(3, Cc), dy=(3, Cc), add=(3, Cc), gamma=(Cc,), beta=(Cc,)).items()}
    o = run_ln(lib, case, inp, dt, expect_rc0=False)
    assert o["rc"] < 0 and "multiple of 8 and at most 2048" in err(lib), (o["rc"], err(lib))
    assert o["ran_fwd"] == (0, 0, 0)
    assert all(b.untouched() for b in o["bufs"])
