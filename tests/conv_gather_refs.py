"""Cases, inputs, references and expected tiles of the implicit-GEMM conv gather tests (tests/test_conv_gather_gpu.py runs
every tile on them through smi_op_conv3x3_ex; tests/test_conv_gather_refs_cpu.py proves without a GPU that the comparison
can fail).  The gather -- which input pixel a row, filter tap and K-tile reads, or the zero page -- is written four times
(csrc/gemm.hip, gemm2.hip twice, gemm3.hip, gemm4.hip three ways); csrc/kernels.h claims that all of them give the same bits.

Two independent references (the CPU file holds them equal):

* reference(): torch in float64 on the 16-bit-rounded inputs -- F.conv2d, after F.interpolate(mode="nearest") for the
  up-sampler, after F.pad(x, (0, 1, 0, 1)) with padding=0 for the VAE encoder's down-sampler, torch.autograd.grad of the
  stride-2 conv for the transposed gradient -- then the epilogue formula of kernels.h;
* gather_reference(): the documented index rule of kernels.h / conv3x3_geom as integer tensors (gather_index: for every
  output row m and tap the input pixel or -1), the patch matrix built from it, one float64 product with the packed filter
  and the same epilogue.  It takes the mutants of the CPU file.

Exactness.  data="int" draws x from {-2..2}, w from {-8..8}, bias / residual / row vector from {-4..4}, xa from {-2..2}, up
from {-4..4} with lora_scale = 0.5.  Every product is an integer of at most 16, a sum over K <= 1152 of them at most 18432,
the epilogue adds at most 12 + 0.5 * 4 * 2 * 4 = 16 in half-integers: every partial sum, in any order and under any
split-K, is an integer or half-integer below 2^15 < 2^24, so fp32 accumulation is exact, nothing overflows fp16, and with
"all fp32, one rounding at the store" (kernels.h) the kernel's output must be torch.equal to reference.to(dt).  No
tolerance.  data="randn" (activations of sigma 1, filter taps of sigma (9 Cin)^-0.5, bias 2, row vector 2, delta 3,
residual 2 as tests/gemm_epilogue_refs.py) serves the `close` bar and the bit comparison between tiles.

Cases (Nb, H, W, Cin, Cout of the FORWARD layer; the transposed cases launch its input gradient: dy on the output grid in,
dx on the input grid out, filter pack_grad(w, flip=False)):

  plain_ragged    3, 5, 7, 128, 320    s1 p1, every term: bias, residual, per-sample row vector (rows_per_vec = 35), rank-4
                                       delta from row 35.  Image boundaries inside a tile, odd W, two K-tiles per tap, M tail
  plain_1x1       2, 1, 1, 64, 64      eight of nine taps masked, two rows
  plain_whole     2, 8, 16, 64, 320    M = 256, N = 320: the smallest launch the 256 x 320 tile takes; two images in a tile
  plain_whole_c128  2, 8, 16, 128, 320 the same with two K-tiles per tap and every term (row vector per 128-pixel sample, delta
                                       on the second sample): the channel offset and the epilogue row rules on the 256 x 320 tile
  plain_handover  33, 16, 16, 64, 2560 264 tiles of 256 x 320 on a persistent grid of one workgroup per CU (256): the
                                       next-tile masks of gemm4.hip, gemm3.hip on many tiles
  plain_handover_ragged  44, 12, 16, 64, 2560  the same grid with 192-pixel images: a tile starts in the middle of an image,
                                       so the next tile's masks differ from the current one's
  s2_odd, s2_even 2, 5, 7 / 2, 6, 8, 64, 64   stride 2 pad 1, Hout = (H + 1) / 2: the last row / column past the odd map
  s2_pad0         2, 6, 8, 64, 64      stride 2 pad 0 (VAE encoder): tap origin (0, 0), bottom / right edges masked
  t_odd, t_even   gradient of s2_odd / s2_even: parity rule, ty < 0, iy < Hin on the last row of an even map
  ups_ragged      2, 3, 5, 64, 64      upsample: >> 1 after the bounds test on the 2x grid
  ups_rows_a / _b 2, 1, 32 / 1, 2, 32, 64, 320   Wout = 64, M = 256: gemm4's row-aligned up-sampling gather
  conv_out_n4     2, 4, 4, 64, 4       the N = 4 column group, fp32 store, bias only
  s2_wide, s2_pad0_wide, t_wide        s2_odd / s2_pad0 at Cout = 160, t_odd at Cin = 320: the strided gathers on the
                                       160-column tiles (N % 160 == 0), which the 64-channel cases cannot reach
  s2_splitk, plain_splitk, t_splitk    s2_even, plain_ragged without the delta, t_even at 128 gathered channels (18
                                       K-tiles), forced ksplit 2, 3, 4 on the "64w" and "128" slice kernels: slices that
                                       start mid-tap and mid-K, four uneven slices

pad = 0 on ODD maps is left out on purpose: conv3x3_out gives (H + 1) / 2 output rows where torch's (0, 1, 0, 1) padding
gives H / 2, and the engine never asks for it (the VAE's maps are even); smi_op_conv3x3_ex refuses it."""
import dataclasses
import functools

import torch
import torch.nn.functional as F

from gemm_epilogue_refs import EPS, MULT, TILES, T128x128_4WAVES, bar  # noqa: F401  (one table of tile codes)

SPLITK_TILES = ("64w", "128")
KSPLITS = (2, 3, 4)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    Nb: int
    H: int
    W: int
    Cin: int
    Cout: int
    mode: str = "plain"     # "plain", "s2", "s2_pad0", "t" (gradient of "s2"), "ups"
    bias: bool = True
    res: bool = True
    rows_per_vec: int = 0   # 0: no row vector
    r: int = 0              # 0: no delta
    row0: int = 0
    out_f32: bool = False
    ksplit: tuple = ()      # forced slice counts (the split-K cases)
    scale: float = 0.5

    # ---- the launch's geometry (what smi_op_conv3x3_ex receives)
    @property
    def stride(self):
        return 2 if self.mode in ("s2", "s2_pad0", "t") else 1

    @property
    def pad(self):
        return 0 if self.mode == "s2_pad0" else 1

    @property
    def upsample(self):
        return int(self.mode == "ups")

    @property
    def transposed(self):
        return int(self.mode == "t")

    @property
    def fwd_out(self):  # output grid of the forward layer (conv3x3_out of kernels.h)
        if self.mode == "plain":
            return self.H, self.W
        if self.mode == "ups":
            return 2 * self.H, 2 * self.W
        return (self.H + 1) // 2, (self.W + 1) // 2

    @property
    def k_in(self):  # (Hin, Win, Cin) of the launch
        return (*self.fwd_out, self.Cout) if self.transposed else (self.H, self.W, self.Cin)

    @property
    def k_out(self):  # (Hout, Wout, Cout) of the launch
        return (self.H, self.W, self.Cin) if self.transposed else (*self.fwd_out, self.Cout)

    @property
    def M(self):
        return self.Nb * self.k_out[0] * self.k_out[1]

    @property
    def N(self):
        return self.k_out[2]

    @property
    def K(self):
        return 9 * self.k_in[2]


CASES = [
    Case("plain_ragged", 3, 5, 7, 128, 320, rows_per_vec=35, r=4, row0=35),
    Case("plain_1x1", 2, 1, 1, 64, 64),
    Case("plain_whole", 2, 8, 16, 64, 320),
    Case("plain_whole_c128", 2, 8, 16, 128, 320, rows_per_vec=128, r=4, row0=128),
    Case("plain_handover", 33, 16, 16, 64, 2560),
    Case("plain_handover_ragged", 44, 12, 16, 64, 2560),
    Case("s2_odd", 2, 5, 7, 64, 64, mode="s2"),
    Case("s2_even", 2, 6, 8, 64, 64, mode="s2"),
    Case("s2_pad0", 2, 6, 8, 64, 64, mode="s2_pad0"),
    Case("t_odd", 2, 5, 7, 64, 64, mode="t"),
    Case("t_even", 2, 6, 8, 64, 64, mode="t"),
    Case("ups_ragged", 2, 3, 5, 64, 64, mode="ups"),
    Case("ups_rows_a", 2, 1, 32, 64, 320, mode="ups"),
    Case("ups_rows_b", 1, 2, 32, 64, 320, mode="ups"),
    Case("conv_out_n4", 2, 4, 4, 64, 4, res=False, out_f32=True),
    Case("s2_wide", 2, 5, 7, 64, 160, mode="s2"),
    Case("s2_pad0_wide", 2, 6, 8, 64, 160, mode="s2_pad0"),
    Case("t_wide", 2, 5, 7, 320, 64, mode="t"),
]
SPLITK_CASES = [
    Case("s2_splitk", 2, 6, 8, 128, 64, mode="s2", ksplit=KSPLITS),
    Case("plain_splitk", 3, 5, 7, 128, 320, rows_per_vec=35, ksplit=KSPLITS),
    Case("t_splitk", 2, 6, 8, 128, 128, mode="t", ksplit=KSPLITS),
]
ALL = CASES + SPLITK_CASES
PLAIN = [c for c in ALL if c.mode == "plain"]


def _cdiv(a, b):
    return (a + b - 1) // b


def heuristic(case):
    """heuristic_tile(p, gemm3=false) of csrc/gemm.hip for a conv: what stands in for a tile that cannot take the launch"""
    M, N = case.M, case.N
    rows256 = _cdiv(M, 256) * _cdiv(N, 128) >= 512
    if N % 160 == 0 and _cdiv(M, 128) * _cdiv(N, 128) >= 1024:
        def cost(bm, bn, eff):
            return _cdiv(_cdiv(M, bm) * _cdiv(N, bn), 256) * bm * bn / eff
        if cost(128, 160, 1.04) < cost(256 if rows256 else 128, 128, 1.10 if rows256 else 1.0):
            return TILES["160"]
    return TILES["256"] if rows256 else TILES["128"]


def expected_tile(case, tile):
    """Code of the tile that runs when `tile` is asked for: gemm2_supported / gemm3_supported / gemm4_supported / fit_tile of
    csrc/gemm*.hip applied by hand.  Every case meets gemm2's layout rules (Cin % 64 == 0; N % 8 == 0, or N == 4 without
    residual and row vector), so v1 runs only when named."""
    code = TILES[tile]
    M, N = case.M, case.N
    plain = case.mode == "plain"
    if tile in ("128", "256", "64w", "v1"):
        return code
    if tile == "64":
        return T128x128_4WAVES                      # the two-wave 64 x 128 tile takes no convs
    if tile == "160":
        return code if N % 8 == 0 else T128x128_4WAVES
    if tile in ("160w", "deep", "64x160"):
        return code if N % 160 == 0 else heuristic(case)
    if tile == "8ph":                                # plain convs only; K = 9 Cin is a multiple of 64 in every case
        return code if plain and N % 8 == 0 else heuristic(case)
    if tile == "5ph":                                # whole 256 x 320 tiles of a plain conv, or of an up-sampler with Wout % 64 == 0
        gather = plain or (case.mode == "ups" and case.k_out[1] % 64 == 0)
        return code if gather and M % 256 == 0 and N % 320 == 0 else heuristic(case)
    raise KeyError(tile)


def pack_fwd(w):
    """[Cout, Cin, 3, 3] -> [Cout, 9 Cin], columns (ky, kx, ci)"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def pack_grad(w, flip):
    """[Cout, Cin, 3, 3] -> [Cin, 9 Cout], columns (ky, kx, co); taps flipped for a stride-1 gradient"""
    wt = w.flip(2, 3) if flip else w
    return wt.permute(1, 2, 3, 0).reshape(w.shape[1], -1).contiguous()


def _randn(g, *shape, std=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float32) * std


def _randint(g, lim, *shape):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def build(case, dt, data):
    """CPU tensors of one case: x (the launch's input image, NHWC), w (the forward layer's torch filter), wp (the packed filter
    the launch reads), bias / res / rowvec in `dt`, xa / up in fp32, and `ref` (float64 [M, N])."""
    assert data in ("int", "randn")
    g = torch.Generator().manual_seed(4321 + sum(map(ord, case.name)) + (data == "randn"))
    integer = data == "int"
    M, N = case.M, case.N
    hin, win, cin = case.k_in

    def draw(lim, std, *shape):
        return _randint(g, lim, *shape) if integer else _randn(g, *shape, std=std)

    d = {"x": draw(2, 1.0, case.Nb, hin, win, cin).to(dt),
         "w": draw(8, (9 * cin) ** -0.5, case.Cout, case.Cin, 3, 3).to(dt)}
    d["wp"] = pack_grad(d["w"], False) if case.transposed else pack_fwd(d["w"])
    d["bias"] = draw(4, 2.0, N).to(dt) if case.bias else None
    d["res"] = draw(4, 2.0, M, N).to(dt) if case.res else None
    d["rowvec"] = draw(4, 2.0, _cdiv(M, case.rows_per_vec), N).to(dt) if case.rows_per_vec else None
    d["xa"] = d["up"] = None
    if case.r:
        d["xa"] = draw(2, 1.0, M - case.row0, case.r)
        d["up"] = draw(4, 3.0 / case.scale * case.r ** -0.5, N, case.r)
    d["ref"] = reference(case, d)
    return d


def epilogue(case, d, c, rowvec_shift=0, row0_shift=0):
    """the epilogue of kernels.h in float64 on c [M, N]; the two shifts are mutants of the CPU file"""
    M = case.M
    if d["bias"] is not None:
        c = c + d["bias"].double()
    if d["rowvec"] is not None:
        idx = ((torch.arange(M, device=c.device) + rowvec_shift) // case.rows_per_vec).clamp(max=d["rowvec"].shape[0] - 1)
        c = c + d["rowvec"].double()[idx]
    if d["xa"] is not None:
        delta = torch.zeros_like(c)
        r0 = case.row0 + row0_shift  # the mutant starts the delta one row late, every row keeps its own xa
        delta[r0:] = case.scale * d["xa"].double()[row0_shift:] @ d["up"].double().t()
        c = c + delta
    if d["res"] is not None:
        c = c + d["res"].double()
    return c


def reference(case, d):
    """float64 [M, N] by torch's own convolution (on whatever device the tensors of d are)"""
    x = d["x"].double().permute(0, 3, 1, 2)
    w = d["w"].double()
    if case.transposed:  # x is dy: the gradient of the stride-2 / pad-1 conv to its input
        xin = torch.zeros(case.Nb, case.Cin, case.H, case.W, dtype=torch.float64, device=x.device, requires_grad=True)
        (y,) = torch.autograd.grad(F.conv2d(xin, w, stride=2, padding=1), xin, x)
    elif case.mode == "ups":
        y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, padding=1)
    elif case.mode == "s2_pad0":
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2, padding=0)
    else:
        y = F.conv2d(x, w, stride=case.stride, padding=1)
    assert tuple(y.shape[2:]) == tuple(case.k_out[:2]), (case.name, y.shape)
    return epilogue(case, d, y.permute(0, 2, 3, 1).reshape(case.M, case.N))


MUTANTS = ("no_mask", "origin", "swap_kykx", "pad0_as_pad1", "t_no_parity", "t_round_up", "ups_halve_first", "img_from_in",
           "rowvec_shift", "row0_shift", "drop_c0")


def gather_index(case, mutant=None):
    """int64 [M, 9]: the input pixel (flat over [Nb, Hin, Win]) that row m reads for tap 3 ky + kx, or -1 for the zero page:
    the rule of csrc/kernels.h (GemmParams / conv3x3_geom) and of the v1 gather.  `mutant` names one deliberate error."""
    hin, win, _ = case.k_in
    hout, wout, _ = case.k_out
    s = case.stride
    pad = 1 if mutant == "pad0_as_pad1" else case.pad
    m = torch.arange(case.M)[:, None]
    tap = torch.arange(9)[None, :]
    ky, kx = tap // 3, tap % 3
    if mutant == "swap_kykx":
        ky, kx = kx, ky
    img = m // (hin * win if mutant == "img_from_in" else hout * wout)
    rem = m % (hout * wout)
    oy, ox = rem // wout, rem % wout
    par = torch.ones(case.M, 9, dtype=torch.bool)
    if case.transposed:
        ty, tx = oy + 1 - ky, ox + 1 - kx
        if mutant == "t_round_up":    # (t + 1) / stride, taking the odd offsets
            iy, ix = (ty + 1) // s, (tx + 1) // s
            par = ((ty + 1) % s == 0) & ((tx + 1) % s == 0)
        else:
            iy, ix = ty // s, tx // s
            par = (iy * s == ty) & (ix * s == tx)
        if mutant == "t_no_parity":
            par = torch.ones_like(par)
        inb = (ty >= 0) & (tx >= 0) & (iy < hin) & (ix < win)
    else:
        o = -pad + (1 if mutant == "origin" else 0)
        iy, ix = oy * s + ky + o, ox * s + kx + o
        if case.upsample:
            if mutant == "ups_halve_first":  # C's truncating / 2 before the test: -1 becomes 0
                iy, ix = torch.div(iy, 2, rounding_mode="trunc"), torch.div(ix, 2, rounding_mode="trunc")
                inb = (iy >= 0) & (ix >= 0) & (iy < hin) & (ix < win)
            else:
                inb = (iy >= 0) & (ix >= 0) & (iy < 2 * hin) & (ix < 2 * win)
                iy, ix = iy >> 1, ix >> 1
        else:
            inb = (iy >= 0) & (ix >= 0) & (iy < hin) & (ix < win)
    idx = img * hin * win + iy * win + ix
    # no_mask: no border test, the read lands wherever the flat index points -- the neighbouring row or image
    ok = par if mutant == "no_mask" else par & inb
    ok = ok & (idx >= 0) & (idx < case.Nb * hin * win)  # (a mutant's index outside the buffer reads as zero)
    return torch.where(ok, idx, torch.full_like(idx, -1))


def gather_reference(case, d, mutant=None):
    """float64 [M, N] from gather_index: patch matrix [M, 9 Cin] x packed filter, then the epilogue"""
    assert mutant is None or mutant in MUTANTS
    cin = case.k_in[2]
    dev = d["x"].device
    idx = gather_index(case, mutant).to(dev)
    x = torch.cat([d["x"].double().reshape(-1, cin), torch.zeros(1, cin, dtype=torch.float64, device=dev)])
    patches = x[idx]                       # [M, 9, Cin]; index -1 is the zero row
    if mutant == "drop_c0":                # every 64-channel K-tile of a tap reads the tap's first 64 channels
        patches = patches[:, :, :64].repeat(1, 1, cin // 64)
    c = patches.reshape(case.M, 9 * cin) @ d["wp"].double().t()
    return epilogue(case, d, c, rowvec_shift=int(mutant == "rowvec_shift"), row0_shift=int(mutant == "row0_shift"))
