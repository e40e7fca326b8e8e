"""Cases, inputs and the float64 reference of the GEMM epilogue tests (tests/test_gemm_epilogue_gpu.py runs the kernels
on them, tests/test_gemm_epilogue_refs_cpu.py proves without a GPU that the comparison can fail).

The reference is the formula of csrc/kernels.h (GemmParams) on the 16-bit-rounded inputs, in float64:

    C[m][n] = sum_k A[m][k] W[n][k] + bias[n] + rowvec[m // rows_per_vec][n]
              + lora_scale * sum_q xa[m - row0][seg(n) r + q] up[n][q]   (rows m >= row0)   + res[m][n]

Term magnitudes (standard deviations): product 0.25, bias 2, row vector 2, delta 3, residual 2, so the sum has sigma ~ 4.6
and its largest element over ~650k is ~ 22.  The bar is 4 eps = 2^-5 (bf16) of that, relative: a whole term missing is
2 / 4.6 = 0.43 in relative norm, 14 bars; a term wrong on ONE row of 1280 elements shows in the largest error, ~ 3.2 sigma of
the term: 9.6 against a bar of 0.69 for the delta, 10.5 for two row vectors' difference.  The CPU file asserts >= 10 bars."""
import dataclasses
import functools

import torch

EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}  # as tests/test_kernels_gpu.py
MULT = 4.0                                                    # close(mult=4): the bar of every GEMM test

# tuner codes of the tiles (csrc/gemm.hip, kTileNames)
TILES = {"128": 1, "256": 2, "64": 14, "64w": 7, "160": 4, "160w": 10, "deep": 11, "64x160": 12, "8ph": 100, "5ph": 200,
         "v1": 300}
T128x128_4WAVES = 13  # what stands in for "160" where N % 8 != 0


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    bias: bool = True
    res: bool = True
    rows_per_vec: int = 0   # 0: no row vector
    ld_rowvec: int = 0      # 0: N
    form: str = ""          # "fwd", "dx" or "" (no delta)
    r: int = 0
    seg: int = 0
    row0: int = 0
    out_f32: bool = False
    ksplit: int = 0
    scale: float = 0.5


WHOLE = dict(M=512, N=1280, K=128)  # 1280 = lcm of the tile widths 128 / 160 / 256 / 320; two 256-row tiles; K = 2 BK
CASES = [
    # every term at once; a row-vector boundary inside a 256-row tile; the row vector a column block of a wider matrix
    Case("whole", **WHOLE, rows_per_vec=128, ld_rowvec=1280 + 8, form="fwd", r=4),
    # batched pass: the last quarter of the rows adapted (row0 inside the second 256-row tile), two fused segments
    Case("batched", **WHOLE, rows_per_vec=128, form="fwd", r=8, seg=640, row0=384),
    Case("dx", **WHOLE, rows_per_vec=128, form="dx", r=12),
    Case("r3", **WHOLE, rows_per_vec=128, form="fwd", r=3),    # the scalar chain
    Case("r16", **WHOLE, rows_per_vec=128, form="fwd", r=16),  # the MFMA delta's limit
    Case("r32", **WHOLE, rows_per_vec=128, form="fwd", r=32),  # past it: the VALU path on every kernel
    Case("f32", **WHOLE, res=False, out_f32=True),
    # partial tiles in M and N for the 128- and 256-wide tiles, N % 8 == 0
    Case("tails", M=520, N=648, K=192, rows_per_vec=104, form="fwd", r=4),
    Case("n4", M=512, N=4, K=128, res=False),
    Case("n4_f32", M=512, N=4, K=128, res=False, out_f32=True),
]
SPLITK = Case("splitk", M=128, N=1280, K=1024, rows_per_vec=32, form="dx", r=12, ksplit=4)
SPLITK_TILES = ("64w", "128")  # the 64 x 128 and 128 x 128 slice kernels


def expected_tile(case, tile):
    """Code of the tile that runs when `tile` is asked for: gemm2_supported / gemm3_supported / gemm4_supported / fit_tile
    of csrc/gemm*.hip applied by hand.  The dense cases here all meet gemm2's alignment rules, none asks for GEGLU, and
    their grids are far below the 512 tiles at which the heuristic leaves the eight-wave 128 x 128 tile."""
    code = TILES[tile]
    M, N, K = case.M, case.N, case.K
    heuristic = TILES["128"]
    if tile in ("128", "256", "64", "64w", "v1"):
        return code                                    # gemm2's 128-wide tiles take N % 8 == 0 and N == 4; v1 N % 4 == 0
    if tile == "160":
        return code if N % 8 == 0 else T128x128_4WAVES
    if tile in ("160w", "deep", "64x160"):
        return code if N % 160 == 0 else heuristic
    if tile == "8ph":
        return code if K % 64 == 0 and N % 8 == 0 and case.seg % 8 == 0 else heuristic
    if tile == "5ph":
        ok = M % 256 == 0 and N % 320 == 0 and K % 64 == 0 and K >= 128 and case.seg % 8 == 0
        return code if ok else heuristic
    raise KeyError(tile)


def _randn(g, *shape, std=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float32) * std


@functools.lru_cache(maxsize=None)
def build(case, dt):
    """CPU tensors of one case: 16-bit operands in `dt`, fp32 delta operands, and `ref` (float64)."""
    g = torch.Generator().manual_seed(1234 + sum(map(ord, case.name)))
    M, N, K = case.M, case.N, case.K
    d = {"A": _randn(g, M, K).to(dt), "W": _randn(g, N, K, std=0.25 * K ** -0.5).to(dt)}
    d["bias"] = _randn(g, N, std=2.0).to(dt) if case.bias else None
    d["res"] = _randn(g, M, N, std=2.0).to(dt) if case.res else None
    d["rowvec"] = None
    if case.rows_per_vec:
        nvec = (M + case.rows_per_vec - 1) // case.rows_per_vec
        d["rowvec"] = _randn(g, nvec, case.ld_rowvec or N, std=2.0).to(dt)
    d["xa"] = d["up"] = None
    if case.form == "fwd":
        nseg = N // case.seg if case.seg else 1
        d["xa"] = _randn(g, M - case.row0, case.r * nseg)
        d["up"] = _randn(g, N, case.r, std=3.0 / case.scale * case.r ** -0.5)
    elif case.form == "dx":
        d["xa"] = _randn(g, M, case.r)
        d["up"] = _randn(g, case.r, N, std=3.0 / case.scale * case.r ** -0.5)  # lora_down [r_tot, N], read transposed
    d["ref"] = reference(case, d)
    return d


def delta(case, d, row_shift=0, swap_segments=False, untransposed=False):
    """[M, N] float64: lora_scale * xa up^T on rows >= row0 - row_shift (mutants: see the CPU test)."""
    M, N = case.M, case.N
    out = torch.zeros(M, N, dtype=torch.float64)
    if not case.form:
        return out
    xa, up = d["xa"].double(), d["up"].double()
    if case.form == "dx":
        upn = up.reshape(N, case.r) if untransposed else up.t()  # up[n][q] = down[q][n]
        return case.scale * xa @ upn.t()
    nseg = N // case.seg if case.seg else 1
    width = case.seg or N
    order = list(range(nseg))
    if swap_segments:
        order[0], order[1] = order[1], order[0]
    r0 = case.row0 - row_shift
    for s in range(nseg):
        x = xa[:, order[s] * case.r:(order[s] + 1) * case.r]
        full = torch.zeros(M, case.r, dtype=torch.float64)
        full[case.row0:] = x
        if row_shift:  # the row below row0 takes the first adapted row's xa
            full[r0:case.row0] = x[:row_shift]
        out[:, s * width:(s + 1) * width] = case.scale * full @ up[s * width:(s + 1) * width].t()
    return out


def reference(case, d, drop=(), rowvec_shift=0, **delta_mut):
    """float64 reference; `drop` names terms to leave out, `rowvec_shift` moves the rows_per_vec boundaries by that many
    rows, the rest goes to delta()."""
    M, N = case.M, case.N
    c = d["A"].double() @ d["W"].double().t()
    if d["bias"] is not None and "bias" not in drop:
        c = c + d["bias"].double()
    if d["rowvec"] is not None and "rowvec" not in drop:
        idx = ((torch.arange(M) + rowvec_shift) // case.rows_per_vec).clamp(max=d["rowvec"].shape[0] - 1)
        c = c + d["rowvec"].double()[idx, :N]
    if "delta" not in drop:
        c = c + delta(case, d, **delta_mut)
    if d["res"] is not None and "res" not in drop:
        c = c + d["res"].double()
    return c


def bar(got, ref, dt):
    """`close` of tests/test_kernels_gpu.py as numbers: (max error / (tol max|ref|), rel-norm error / tol); it passes when
    both are <= 1."""
    got, ref = got.double(), ref.double()
    tol = EPS[dt] * MULT
    err = (got - ref).abs().max().item()
    rel = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    return err / (tol * (ref.abs().max().item() + 1e-6)), rel / tol
