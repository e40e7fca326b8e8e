"""Oracle for LPIPS (AlexNet, v0.1): the metric restated in plain torch (`F.conv2d`, `F.max_pool2d`) in fp64 on the CPU.
Shared by test_lpips_cpu.py, test_lpips_gpu.py and test_lpips_score_gpu.py; never imported by the product.  Neither the
`lpips` nor the `torchvision` package is installed here, so the restatement follows their published definition.

The storage-dtype twin is the same forward with the weights in the dtype and a rounding to the dtype at exactly the
engine's storage sites: the scaled input, every layer output (the pre-activation the GEMM stores) and every pooled map.
Everything between two sites stays fp64, as the engine's stays fp32.

The bar of a dtype is 2 x the twin's distance from fp64 on the same inputs and weights.  The factor 2 is the project's
own (tests/clip_vision_refs.py), for the same reason: the engine's roundings fall at the same sites but on fp32 sums.
It is computed here from the reference alone -- never from the engine's output -- and printed by the tests.

Three metrics: relative L2 of each tap's features; relative L2 over a batch's vector of distances; per pair, the ABSOLUTE
error against 2 x the twin's largest absolute error in that batch (the twin's absolute error is nearly constant across
pairs whose distances span three decades, so a relative per-pair bar would be set by the smallest pair alone)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
GEOMETRY = ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))
CONVS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
ALEX = (64, 192, 384, 256, 256)
NETS = ("tiny_alex", "alex")
SIZES = ((64, 64), (31, 31), (64, 80))  # (H, W): the script's size, the smallest legal one, a non-square one
MAP_SIZES = {(64, 64): [(15, 15), (7, 7), (3, 3), (3, 3), (3, 3)],
             (31, 31): [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)],
             (64, 80): [(15, 19), (7, 9), (3, 4), (3, 4), (3, 4)]}
AMPLITUDES = (2, 1, 0.3, 0.1, 0.03, 0.01)  # of the perturbation, in the [-1, 1] units of the network's input
MUTATIONS = ("no_scaling", "channels_reversed", "tap_after_pool", "pool_stride1", "no_bias", "no_relu",
             "skip_last_layer", "no_unit_normalise", "abs_instead_of_square", "lin_uniform")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


@functools.lru_cache(maxsize=None)
def weights(net):
    """the product's seeded synthetic weights as an fp64 state dict (bf16-representable values)"""
    from sliders_conceptmod_amd import model_util
    return {k: v.detach().double() for k, v in model_util.load_lpips(f"synthetic://{net}").state_dict().items()}


@functools.lru_cache(maxsize=None)
def pairs_u8(size, seed=0):
    """(a, b) uint8 [6, H, W, 3]: pair j's b is a + AMPLITUDES[j] x uniform noise, clipped and rounded to uint8"""
    H, W = size
    rs = np.random.RandomState(1000 * H + W + seed)
    a = rs.randint(0, 256, (len(AMPLITUDES), H, W, 3)).astype(np.float64)
    amp = np.asarray(AMPLITUDES, dtype=np.float64).reshape(-1, 1, 1, 1) * 127.5
    b = np.clip(np.rint(a + amp * rs.uniform(-1, 1, a.shape)), 0, 255)
    assert all((a[j] != b[j]).any() for j in range(len(AMPLITUDES)))
    return torch.from_numpy(a.astype(np.uint8)), torch.from_numpy(b.astype(np.uint8))


def to_input(u8):
    """uint8 [n, H, W, 3] -> fp64 [n, 3, H, W] in [-1, 1]"""
    return u8.permute(0, 3, 1, 2).double() / 127.5 - 1.0


def forward(sd, in0, in1, dtype=None, mutation=None):
    """(taps: five post-ReLU maps fp64 [2n, C, Ho, Wo], per_layer fp64 [n, 5], dist fp64 [n]) of LPIPS on fp64 inputs in
    [-1, 1].  dtype: the storage-dtype twin.  mutation: one deliberate mistake (MUTATIONS)."""
    q = (lambda t: t.to(dtype).double()) if dtype is not None else (lambda t: t)
    n = in0.shape[0]
    x = torch.cat([in0, in1]).double()
    if mutation == "channels_reversed":
        x = x.flip(1)
    if mutation != "no_scaling":
        x = (x - torch.tensor(SHIFT).double().view(1, 3, 1, 1)) / torch.tensor(SCALE).double().view(1, 3, 1, 1)
    x = q(x)
    relu = (lambda t: t) if mutation == "no_relu" else F.relu
    taps = []
    for i, (name, (k, s, p)) in enumerate(zip(CONVS, GEOMETRY)):
        b = None if mutation == "no_bias" else q(sd[name + ".bias"])
        y = q(F.conv2d(x, q(sd[name + ".weight"]), b, stride=s, padding=p))  # the stored pre-activation
        x = relu(y)
        pooled = q(F.max_pool2d(x, 3, 1 if mutation == "pool_stride1" else 2)) if i < 2 else None
        taps.append(pooled if (mutation == "tap_after_pool" and i < 2) else x)
        if pooled is not None:
            x = pooled
    per_layer = []
    for i, f in enumerate(taps):
        w = q(sd[f"lin{i}.model.1.weight"]).view(1, -1, 1, 1)
        if mutation == "lin_uniform":
            w = torch.full_like(w, w.mean().item())
        if mutation != "no_unit_normalise":
            f = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        d = f[:n] - f[n:]
        d = d.abs() if mutation == "abs_instead_of_square" else d * d
        per_layer.append((d * w).sum(1).mean((1, 2)))
    per_layer = torch.stack(per_layer, 1)
    if mutation == "skip_last_layer":
        per_layer = per_layer[:, :4]
    return taps, per_layer, per_layer.sum(1)


@functools.lru_cache(maxsize=None)
def reference(net, size):
    """fp64 (taps, per_layer, dist) on pairs_u8(size); computed once, never modified"""
    a, b = pairs_u8(size)
    return forward(weights(net), to_input(a), to_input(b))


@functools.lru_cache(maxsize=None)
def twin(net, size, dtype):
    a, b = pairs_u8(size)
    return forward(weights(net), to_input(a), to_input(b), dtype=dtype)


@functools.lru_cache(maxsize=None)
def bars(net, size, dtype):
    """{'taps': [5 relative-L2 bars], 'per_layer': [5], 'batch': relative L2 over the distances, 'pair_abs': absolute}
    = 2 x the twin's own distance from fp64"""
    ref, low = reference(net, size), twin(net, size, dtype)
    return {"taps": [2 * rel(l, r) for l, r in zip(low[0], ref[0])],
            "per_layer": [2 * rel(low[1][:, t], ref[1][:, t]) for t in range(5)],
            "batch": 2 * rel(low[2], ref[2]),
            "pair_abs": 2 * (low[2] - ref[2]).abs().max().item()}


def mutated_batch_distance(net, size, mutation):
    """relative L2 over the batch's distances between the mutated and the true metric, in fp64"""
    a, b = pairs_u8(size)
    return rel(forward(weights(net), to_input(a), to_input(b), mutation=mutation)[2], reference(net, size)[2])
