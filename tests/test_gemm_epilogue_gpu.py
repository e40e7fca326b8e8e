"""Every epilogue term on every GEMM tile, at kernel level (smi_op_gemm_epilogue launches a NAMED tile in-process and
reports which tile really ran).  The epilogue arithmetic has one definition (csrc/gemm_epilogue.h) that every kernel
generation and the split-K finish call; this file is the check that they do, on the classes the generation digest of
tests/test_kernels_gpu.py does not reach at kernel level: the row vector, the dX-form delta, ranks off the vector paths,
the N == 4 group, the batched-pass row rule inside a tile.

For every case of tests/gemm_epilogue_refs.py, both 16-bit types and every tile code:
  (a) the result meets `close` of tests/test_kernels_gpu.py (EPS[dt] * 4) against the float64 reference;
  (b) it is torch.equal to the 128 x 128 tile's result;
  (c) the tile that ran is the one gemm_epilogue_refs.expected_tile names -- a fallback the table does not list fails.
Forced split-K (four slices on both slice kernels) is held to the rule of tools/check_splitk.py against the un-split kernel:
fp32 to 3e-6 of the largest element, 16-bit to a last-bit flip.
tests/test_gemm_epilogue_refs_cpu.py proves, on the same inputs, that (a) rejects every single-term mutation."""
import ctypes as C

import pytest
import torch

import gemm_epilogue_refs as GR
from test_kernels_gpu import P, chk, close, dcode

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def lib():
    from sliders_conceptmod_amd import _native
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return _native.lib()


_dev = {}


def on_gpu(case, dt):
    """the case's operands on the GPU, uploaded once and never written"""
    if (case, dt) not in _dev:
        _dev[(case, dt)] = {k: (None if v is None else v.cuda()) for k, v in GR.build(case, dt).items()}
    return _dev[(case, dt)]


def run(lib, case, dt, tile_code, ksplit=0, out_f32=None):
    d = on_gpu(case, dt)
    f32 = case.out_f32 if out_f32 is None else out_f32
    c = torch.full((case.M, case.N), float("nan"), device="cuda", dtype=torch.float32 if f32 else dt)
    ran = C.c_int(-1)
    xa = d["xa"]
    chk(lib, lib.smi_op_gemm_epilogue(
        dcode(dt), P(d["A"]), P(d["W"]), P(c), case.M, case.N, case.K, int(f32), P(d["bias"]), P(d["res"]),
        P(d["rowvec"]), max(case.rows_per_vec, 1), case.ld_rowvec, P(xa), 0 if xa is None else xa.shape[1], P(d["up"]),
        case.r, case.seg, case.row0, case.scale, int(case.form == "dx"), tile_code, ksplit, C.byref(ran), None))
    torch.cuda.synchronize()
    return c, ran.value


@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", GR.CASES, ids=[c.name for c in GR.CASES])
def test_every_tile_computes_the_same_epilogue(lib, case, dt):
    ref = on_gpu(case, dt)["ref"]
    base, ran = run(lib, case, dt, GR.TILES["128"])
    assert ran == GR.TILES["128"]
    failures = []
    for tile, code in GR.TILES.items():
        got, ran = run(lib, case, dt, code)
        want = GR.expected_tile(case, tile)
        if ran != want:
            failures.append(f"{tile}: tile {ran} ran, expected {want}")
        try:
            close(got, ref, dt, what=f"{case.name} on {tile}")
        except AssertionError as e:
            failures.append(str(e))
        if not torch.equal(got, base):
            diff = (got.float() - base.float()).abs()
            failures.append(f"{tile}: {int((diff > 0).sum())} elements differ from the 128 x 128 tile's, max {diff.max().item():.3e}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
def test_launch_gemm_own_choice_matches(lib, dt):
    """tile code 0 is launch_gemm itself (heuristic / tuner / split-K rule): same bits as the named tile, reported as 0"""
    case = GR.CASES[0]
    base, _ = run(lib, case, dt, GR.TILES["128"])
    got, ran = run(lib, case, dt, 0)
    assert ran == 0 and torch.equal(got, base)


@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
def test_forced_splitk_matches_the_unsplit_kernel(lib, dt):
    case = GR.SPLITK
    ref = on_gpu(case, dt)["ref"]
    scratch = torch.empty(case.ksplit * case.M * case.N * 4, dtype=torch.uint8, device="cuda")
    chk(lib, lib.smi_op_gemm_scratch(P(scratch), scratch.numel()))
    try:
        base32, _ = run(lib, case, dt, GR.TILES["128"], out_f32=True)
        base16, _ = run(lib, case, dt, GR.TILES["128"], out_f32=False)
        close(base16, ref, dt, what="un-split")
        for tile in GR.SPLITK_TILES:
            got32, ran = run(lib, case, dt, GR.TILES[tile], ksplit=case.ksplit, out_f32=True)
            assert ran == GR.TILES[tile]
            e = ((got32 - base32).abs().max() / base32.abs().max()).item()
            assert torch.isfinite(got32).all() and e < 3e-6, (tile, e)
            got16, ran = run(lib, case, dt, GR.TILES[tile], ksplit=case.ksplit, out_f32=False)
            assert ran == GR.TILES[tile]
            close(got16, ref, dt, what=f"split-K on {tile}")
            # one 16-bit rounding of sums that differ by fp32 summation order: a rare last-bit flip
            flip = (got16.float() - base16.float()).abs().max().item()
            assert flip <= GR.EPS[dt] * base16.float().abs().max().item() * 2, (tile, flip)
        # the two slice kernels add the same K-tiles in the same order: the same bits
        a, _ = run(lib, case, dt, GR.TILES["64w"], ksplit=case.ksplit, out_f32=True)
        b, _ = run(lib, case, dt, GR.TILES["128"], ksplit=case.ksplit, out_f32=True)
        assert torch.equal(a, b)
    finally:
        chk(lib, lib.smi_op_gemm_scratch(None, 0))


def test_unknown_tile_code_is_an_error(lib):
    case = GR.CASES[0]
    d = on_gpu(case, torch.float16)
    c = torch.empty(case.M, case.N, device="cuda", dtype=torch.float16)
    ran = C.c_int(-1)
    rc = lib.smi_op_gemm_epilogue(0, P(d["A"]), P(d["W"]), P(c), case.M, case.N, case.K, 0, None, None, None, 1, 0, None, 0,
                                  None, 0, 0, 0, 0.0, 0, 9999, 0, C.byref(ran), None)
    assert rc != 0 and b"unknown tile code" in lib.smi_last_error()
