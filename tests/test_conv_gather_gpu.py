"""The implicit-GEMM conv gather on every GEMM tile, per element (smi_op_conv3x3_ex launches a 3x3 conv of any gather mode
on a NAMED tile in-process and reports which tile really ran).  Which input pixel a row, filter tap and K-tile reads -- or
the zero page -- is written once in csrc/gemm.hip (v1), twice in gemm2.hip (plain stride-1 fast path, general path), once in
gemm3.hip (tap masks) and three ways in gemm4.hip (tap masks with a next-tile copy, the row-aligned up-sampling gather, the
2x2 grid); the tests of tests/test_kernels_gpu.py see the one or two tiles launch_gemm picks at their sizes, through a norm.

For every case of tests/conv_gather_refs.py, both 16-bit types, tile code 0 (launch_gemm's own choice) without and with
split-K scratch, and every tile code:
  integer data  the result is torch.equal to the float64 reference rounded once (fp32 accumulation of these integers and
                half-integers is exact in any order, conv_gather_refs.py), and the tile that ran is the one
                conv_gather_refs.expected_tile names -- a fallback the table does not list fails;
  random data   `close` of tests/test_kernels_gpu.py (EPS[dt] * 4) against float64, every tile torch.equal to the 128 x 128
                tile's result, code 0 too; code 0 with scratch, where the split-K rule may fire, `close` plus a last-bit flip.
Forced split-K (2, 3, 4 slices of 18 K-tiles on both slice kernels, strided and transposed gathers included): exact on the
integers, and on random data the rule of test_gemm_epilogue_gpu.test_forced_splitk_matches_the_unsplit_kernel.
tests/test_conv_gather_refs_cpu.py proves on the same inputs that eleven single errors of the index rule each fail both
comparisons."""
import ctypes as C

import pytest
import torch

import conv_gather_refs as CR
from test_kernels_gpu import P, chk, close, dcode

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]


@pytest.fixture(scope="module")
def lib():
    from sliders_conceptmod_amd import _native
    assert torch.cuda.is_available(), "these tests need the GPU box"
    yield _native.lib()
    _dev.clear()  # (the hand-over cases hold a few hundred MB of float64 reference each)


_dev = {}


def on_gpu(case, dt, data):
    """the case's operands on the GPU, uploaded once and never written; `want`: the reference as the kernel stores it"""
    key = (case, dt, data)
    if key not in _dev:
        d = dict(CR.build(case, dt, data))
        d["want"] = d["ref"].float() if case.out_f32 else d["ref"].to(dt)
        _dev[key] = {k: (None if v is None else v.cuda()) for k, v in d.items()}
    return _dev[key]


def launch(lib, case, dt, d, out, tile_code, ksplit=0, **over):
    """one smi_op_conv3x3_ex call with the case's arguments (`over` replaces some, for the error cases); returns (rc, ran)"""
    hin, win, cin = case.k_in
    hout, wout, cout = case.k_out
    a = dict(nb=case.Nb, hin=hin, win=win, cin=cin, cout=cout, stride=case.stride, upsample=case.upsample,
             transposed=case.transposed, hout=hout, wout=wout, pad=case.pad)
    a.update(over)
    ran = C.c_int(-1)
    xa = d["xa"]
    rc = lib.smi_op_conv3x3_ex(
        dcode(dt), P(d["x"]), P(d["wp"]), P(d["bias"]), P(out), a["nb"], a["hin"], a["win"], a["cin"], a["cout"], a["stride"],
        a["upsample"], a["transposed"], a["hout"], a["wout"], a["pad"], int(out.dtype == torch.float32), P(d["res"]),
        P(d["rowvec"]), max(case.rows_per_vec, 1), 0, P(xa), 0 if xa is None else xa.shape[1], P(d["up"]), case.r, case.row0,
        case.scale, tile_code, ksplit, C.byref(ran), None)
    return rc, ran.value


def run(lib, case, dt, data, tile_code, ksplit=0, out_f32=None):
    d = on_gpu(case, dt, data)
    f32 = case.out_f32 if out_f32 is None else out_f32
    out = torch.full((case.M, case.N), float("nan"), device="cuda", dtype=torch.float32 if f32 else dt)
    rc, ran = launch(lib, case, dt, d, out, tile_code, ksplit)
    chk(lib, rc)
    torch.cuda.synchronize()
    return out, ran


def differs(got, want):
    bad = ~(got == want)  # (NaN left from the pre-fill counts)
    n = int(bad.sum())
    if not n:
        return ""
    m = int(bad.any(dim=1).nonzero()[0])
    return f"{n} elements differ, first in row {m}, max {(got.double() - want.double()).abs().nan_to_num(nan=float('inf')).max().item():.3e}"


def last_bit(got, base, dt):
    """one 16-bit rounding of sums that differ by fp32 summation order: a rare last-bit flip"""
    flip = (got.float() - base.float()).abs().max().item()
    return flip <= CR.EPS[dt] * base.float().abs().max().item() * 2, flip


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("case", CR.ALL, ids=[c.name for c in CR.ALL])
def test_every_tile_reads_the_same_pixels(lib, case, dt):
    failures = []
    # split-K scratch for the rule (at most 16 slices; the rule takes what fits)
    scratch = torch.empty(min(16 * case.M * case.N * 4, 64 << 20), dtype=torch.uint8, device="cuda")
    for data in ("int", "randn"):
        d = on_gpu(case, dt, data)
        ref, want = d["ref"], d["want"]
        base = None
        if data == "randn":
            base, ran = run(lib, case, dt, data, CR.TILES["128"])
            assert ran == CR.TILES["128"]
        runs = [("own choice", 0, False), ("own choice with scratch", 0, True)] + [(t, c, False) for t, c in CR.TILES.items()]
        for what, code, lend in runs:
            if lend:
                chk(lib, lib.smi_op_gemm_scratch(P(scratch), scratch.numel()))
            try:
                got, ran = run(lib, case, dt, data, code)
            finally:
                if lend:
                    chk(lib, lib.smi_op_gemm_scratch(None, 0))
            tag = f"{case.name} {data} on {what}"
            expect = 0 if code == 0 else CR.expected_tile(case, what)
            if ran != expect:
                failures.append(f"{tag}: tile {ran} ran, expected {expect}")
            if data == "int":
                bad = differs(got, want)
                if bad:
                    failures.append(f"{tag} (ran {ran}): {bad}")
                continue
            try:
                close(got, ref, dt, what=tag)
            except AssertionError as e:
                failures.append(str(e))
            if lend:
                ok, flip = last_bit(got, base, dt)
                if not ok:
                    failures.append(f"{tag}: {flip:.3e} from the un-split result, more than a last-bit flip")
            elif not torch.equal(got, base):
                failures.append(f"{tag} (ran {ran}) against the 128 x 128 tile: {differs(got, base)}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("case", CR.SPLITK_CASES, ids=[c.name for c in CR.SPLITK_CASES])
def test_forced_splitk_slices_start_mid_tap(lib, case, dt):
    failures = []
    scratch = torch.empty(max(case.ksplit) * case.M * case.N * 4, dtype=torch.uint8, device="cuda")
    chk(lib, lib.smi_op_gemm_scratch(P(scratch), scratch.numel()))
    try:
        d = on_gpu(case, dt, "int")
        for S in case.ksplit:
            for tile in CR.SPLITK_TILES:
                for f32 in (False, True):
                    got, ran = run(lib, case, dt, "int", CR.TILES[tile], ksplit=S, out_f32=f32)
                    tag = f"{case.name} int, {S} slices on {tile}, {'fp32' if f32 else '16-bit'}"
                    if ran != CR.TILES[tile]:
                        failures.append(f"{tag}: tile {ran} ran")
                    bad = differs(got, d["ref"].float() if f32 else d["ref"].to(dt))
                    if bad:
                        failures.append(f"{tag}: {bad}")
        ref = on_gpu(case, dt, "randn")["ref"]
        base32, _ = run(lib, case, dt, "randn", CR.TILES["128"], out_f32=True)
        base16, _ = run(lib, case, dt, "randn", CR.TILES["128"], out_f32=False)
        close(base16, ref, dt, what="un-split")
        for S in case.ksplit:
            got = {}
            for tile in CR.SPLITK_TILES:
                tag = f"{case.name} randn, {S} slices on {tile}"
                got32, ran = run(lib, case, dt, "randn", CR.TILES[tile], ksplit=S, out_f32=True)
                assert ran == CR.TILES[tile]
                got[tile] = got32
                e = ((got32 - base32).abs().max() / base32.abs().max()).item()
                if not (bool(torch.isfinite(got32).all()) and e < 3e-6):
                    failures.append(f"{tag}: fp32 {e:.3e} of the largest element from the un-split kernel")
                got16, ran = run(lib, case, dt, "randn", CR.TILES[tile], ksplit=S, out_f32=False)
                assert ran == CR.TILES[tile]
                try:
                    close(got16, ref, dt, what=tag)
                except AssertionError as e:
                    failures.append(str(e))
                ok, flip = last_bit(got16, base16, dt)
                if not ok:
                    failures.append(f"{tag}: {flip:.3e} from the un-split result, more than a last-bit flip")
            # the two slice kernels add the same K-tiles in the same order: the same bits
            if not torch.equal(got["64w"], got["128"]):
                failures.append(f"{case.name} randn, {S} slices: the slice kernels differ: {differs(got['64w'], got['128'])}")
    finally:
        chk(lib, lib.smi_op_gemm_scratch(None, 0))
    assert not failures, "\n".join(failures)


BY = {c.name: c for c in CR.ALL}


BAD = [
    ("unknown tile code", "plain_whole", 9999, {}, b"unknown tile code"),
    # the output grid is not the one the input grid and the mode give
    ("one output row too many", "plain_whole", 1, dict(hout=9), b"inconsistent geometry"),
    ("stride-2 output grid on a plain conv", "s2_even", 1, dict(stride=1), b"inconsistent geometry"),
    ("dy grid of another map", "t_even", 1, dict(hin=4), b"inconsistent geometry"),
    # the geometry checks of launch_gemm hold for a named tile too
    ("stride 3 on a named tile", "plain_whole", 1, dict(stride=3), b"inconsistent geometry"),
    ("stride 3 on the launcher's own choice", "plain_whole", 0, dict(stride=3), b"inconsistent geometry"),
    ("pad 0 on an odd map", "s2_odd", 1, dict(pad=0), b"even map"),
    ("pad 2", "plain_whole", 1, dict(pad=2), b"pad=2"),
    ("up-sampling at stride 2", "s2_even", 1, dict(upsample=1), b"upsample"),
]


@pytest.mark.parametrize("what,name,code,over,msg", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_bad_arguments_are_refused_before_any_launch(lib, what, name, code, over, msg):
    case, dt = BY[name], torch.float16
    d = on_gpu(case, dt, "int")
    # (sized for the refused geometry as well: nothing may be written, but nothing could land outside either)
    out = torch.full((2 * case.M, case.N), float("nan"), device="cuda", dtype=dt)
    rc, ran = launch(lib, case, dt, d, out, code, **over)
    torch.cuda.synchronize()
    assert rc < 0 and msg in lib.smi_last_error(), (what, rc, lib.smi_last_error())
    assert bool(torch.isnan(out).all()), what
