"""Python reference of the up-sampler conv's phase form (csrc/engine.hip
pack_conv_phase_kernel, csrc/kernels.h conv2x2_phase, csrc/elementwise.hip copy_cols_phase_kernel).

`conv2d(interpolate(x, 2, 'nearest'), w, b, padding=1)`: output pixel (2i + a, 2j + b), a, b in {0, 1}, sees only the 2x2
low-res pixels of rows {i - 1 + a, i + a} and columns {j - 1 + b, j + b} (zero outside the map), so each of the four phases
is a same-size 2x2 conv with tap origin (a - 1, b - 1) whose weights are sums of the 3x3 weights.  Its adjoint is one
4x4 / stride-2 / pad-1 conv over dy (grad_filter_4x4).  Everything here works in the dtype it is given (the CPU test
gives float64)."""
import torch
import torch.nn.functional as F

# (phase a, tap p) -> the 3x3 rows (or columns) that land on low-res row i - 1 + a + p
TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
SHAPES = [(1, 1), (1, 4), (2, 3), (5, 7)]  # H x W: at 1 x 1 every tap but one is padding
BATCHES = [1, 3]


def upconv_ref(x, w, b):
    """x [Nb, Cin, H, W] -> [Nb, Cout, 2H, 2W]: what the layer computes"""
    return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)


def phase_filters(w):
    """w [Cout, Cin, 3, 3] -> [4, Cout, Cin, 2, 2]: filter of phase 2a + b, exact sums"""
    out = w.new_zeros(4, w.shape[0], w.shape[1], 2, 2)
    for a in range(2):
        for b in range(2):
            for p in range(2):
                for q in range(2):
                    for ky in TAPS[(a, p)]:
                        for kx in TAPS[(b, q)]:
                            out[2 * a + b, :, :, p, q] += w[:, :, ky, kx]
    return out


def phase_pack(w, dtype=None):
    """the engine's phase pack [4][Cout][4 * Cin], tap-major / channel order; summed in w's dtype, rounded once to `dtype`"""
    f = phase_filters(w).permute(0, 1, 3, 4, 2).reshape(4, w.shape[0], -1)
    return f.to(dtype) if dtype is not None else f


def phase_planes(x, w, b):
    """x [Nb, H, W, Cin] (NHWC) -> phase-major [4, Nb, H, W, Cout]: plane 2a + b holds the output pixels (2i + a, 2j + b)"""
    nb, H, W, cin = x.shape
    f = phase_filters(w)
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))  # low-res pixel (r, c) at padded (r + 1, c + 1)
    planes = []
    for a in range(2):
        for bb in range(2):
            win = xp[:, :, a:a + H + 1, bb:bb + W + 1]  # rows i - 1 + a .. i + a for i in [0, H)
            y = F.conv2d(win, f[2 * a + bb], b)
            planes.append(y.permute(0, 2, 3, 1))
    return torch.stack(planes)


def unshuffle(planes):
    """phase-major [4, Nb, H, W, C] -> [Nb, 2H, 2W, C]: the row order the concat's shuffling copy writes"""
    _, nb, H, W, c = planes.shape
    return planes.view(2, 2, nb, H, W, c).permute(2, 3, 0, 4, 1, 5).reshape(nb, 2 * H, 2 * W, c)


def shuffle(y):
    """inverse of unshuffle: [Nb, 2H, 2W, C] -> [4, Nb, H, W, C]"""
    nb, H2, W2, c = y.shape
    return y.view(nb, H2 // 2, 2, W2 // 2, 2, c).permute(2, 4, 0, 1, 3, 5).reshape(4, nb, H2 // 2, W2 // 2, c)


def grad_filter_4x4(w):
    """w [Cout, Cin, 3, 3] -> k [Cin, Cout, 4, 4] with dx = conv2d(dy, k, stride=2, padding=1): row tap u reads dy row
    2r - 1 + u and carries phase / tap (a, p) = (1, 1), (0, 1), (1, 0), (0, 0) for u = 0..3; columns alike"""
    ap = [(1, 1), (0, 1), (1, 0), (0, 0)]
    k = w.new_zeros(w.shape[1], w.shape[0], 4, 4)
    for u, (a, p) in enumerate(ap):
        for v, (b, q) in enumerate(ap):
            for ky in TAPS[(a, p)]:
                for kx in TAPS[(b, q)]:
                    k[:, :, u, v] += w[:, :, ky, kx].t()
    return k


def upconv_dx_4x4(dy, w):
    """dy [Nb, Cout, 2H, 2W] -> dx [Nb, Cin, H, W], the adjoint of upconv_ref in one conv on the input grid"""
    return F.conv2d(dy, grad_filter_4x4(w), stride=2, padding=1)
