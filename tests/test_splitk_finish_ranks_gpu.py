"""The split-K finish kernel with the delta's rank as a compile-time constant (csrc/gemm.hip, splitk_finish_kernel<T, NS, LR>:
ranks 12 and 24, the dX of the fused q|k|v projections at adaptor rank 4 and 8) against the un-split kernel, BIT FOR BIT.

A and W hold small integers (|a|, |w| <= 2, K = 1024: every partial sum is an integer below 2^13), so the fp32 accumulation
is exact in any order and the split result may differ from the un-split one only through the epilogue.  Bias, row vector,
the rank-r delta (fp32 operands with full mantissas: its fmaf chain rounds at every step) and the residual follow in the
order of csrc/gemm_epilogue.h on both sides; any other order or grouping of the delta's chain shows as different bits.
Ranks 4 and 8 (unrolled inside the common finish kernel) and 16 (the rolled scalar chain) run through the same check."""
import ctypes as C

import pytest
import torch

from test_kernels_gpu import P, chk, dcode

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
M, N, K = 200, 1280, 1024      # a ragged last row tile; 16 K-tiles
TILE_128, TILE_64W = 1, 7      # tuner codes of the two slice kernels (csrc/gemm.hip, kTileNames)


@pytest.fixture(scope="module")
def lib():
    from sliders_conceptmod_amd import _native
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return _native.lib()


@pytest.fixture(scope="module")
def scratch(lib):
    ws = torch.empty(4 * M * N * 4, dtype=torch.uint8, device="cuda")
    chk(lib, lib.smi_op_gemm_scratch(P(ws), ws.numel()))
    yield ws
    chk(lib, lib.smi_op_gemm_scratch(None, 0))


_inputs = {}


def inputs(dt):
    """operands on the GPU, made once per type and never written"""
    if dt not in _inputs:
        g = torch.Generator().manual_seed(7)
        d = {"A": torch.randint(-2, 3, (M, K), generator=g).to(dt), "W": torch.randint(-2, 3, (N, K), generator=g).to(dt),
             "bias": (torch.randn(N, generator=g) * 2).to(dt), "res": (torch.randn(M, N, generator=g) * 2).to(dt),
             "rowvec": (torch.randn((M + 31) // 32, N, generator=g) * 2).to(dt)}
        for r in (4, 8, 12, 16, 24):
            d[f"xa{r}"] = torch.randn(M, r, generator=g)
            d[f"down{r}"] = torch.randn(r, N, generator=g) * r ** -0.5   # dX form: lora_down [r, N], read transposed
            d[f"up{r}"] = torch.randn(N, r, generator=g) * r ** -0.5     # forward form: lora_up [N, r]
        _inputs[dt] = {k: v.cuda() for k, v in d.items()}
    return _inputs[dt]


def run(lib, dt, r, dx, f32, tile, ksplit):
    d = inputs(dt)
    c = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float32 if f32 else dt)
    ran = C.c_int(-1)
    chk(lib, lib.smi_op_gemm_epilogue(
        dcode(dt), P(d["A"]), P(d["W"]), P(c), M, N, K, int(f32), P(d["bias"]), P(d["res"]), P(d["rowvec"]), 32, 0,
        P(d[f"xa{r}"]), r, P(d[f"down{r}" if dx else f"up{r}"]), r, 0, 0, 0.375, int(dx), tile, ksplit, C.byref(ran), None))
    torch.cuda.synchronize()
    assert ran.value == tile
    return c


@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
@pytest.mark.parametrize("r,dx", [(12, True), (24, True), (12, False), (4, True), (8, True), (16, True)],
                         ids=["dx12", "dx24", "fwd12", "dx4", "dx8", "dx16"])
def test_finish_delta_chain_matches_the_unsplit_kernel_bitwise(lib, scratch, dt, r, dx):
    d = inputs(dt)
    for f32 in (True, False):
        base = run(lib, dt, r, dx, f32, TILE_128, 0)
        # the un-split result itself against float64 (exact product, so only the epilogue's roundings remain)
        delta = d[f"xa{r}"].double() @ (d[f"down{r}"].double() if dx else d[f"up{r}"].double().t())
        ref = (d["A"].double() @ d["W"].double().t() + d["bias"].double() + d["rowvec"].double().repeat_interleave(32, 0)[:M]
               + 0.375 * delta + d["res"].double())
        tol = 1e-5 if f32 else (2.0 ** -10 if dt == torch.float16 else 2.0 ** -7)
        assert ((base.double() - ref).abs().max() / ref.abs().max()).item() < tol
        for tile in (TILE_64W, TILE_128):
            for ksplit in (3, 4):
                got = run(lib, dt, r, dx, f32, tile, ksplit)
                diff = (got.float() - base.float()).abs()
                assert torch.equal(got, base), (f"rank {r} {'dx' if dx else 'fwd'} f32={f32} tile {tile} S={ksplit}: "
                                                f"{int((diff > 0).sum())} elements differ, max {diff.max().item():.3e}")
