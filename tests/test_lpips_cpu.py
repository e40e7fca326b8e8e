"""LPIPS without a GPU: the reference's own properties, the mutation condition against the bars, and the host logic of
the container, the loader and the `lpips_score` command."""
import math
import os

import numpy as np
import pytest
import torch

from tests import lpips_refs as R

DTYPES = (torch.float16, torch.bfloat16)


def test_parameter_counts():
    from sliders_conceptmod_amd import model_util
    m = model_util.load_lpips("synthetic://alex")
    convs = sum(p.numel() for k, p in m.named_parameters() if k.startswith("net."))
    lins = sum(p.numel() for k, p in m.named_parameters() if k.startswith("lin"))
    assert convs == 2469696 and lins == 1152
    assert sum(p.numel() for p in m.parameters()) == convs + lins
    for i, c in enumerate(R.ALEX):
        assert tuple(m.state_dict()[f"lin{i}.model.1.weight"].shape) == (1, c, 1, 1)
        assert (m.state_dict()[f"lin{i}.model.1.weight"] >= 0).all()
    # bf16-representable, so that fp16 and bf16 engines (and the fp64 reference) hold the same numbers
    for k, p in m.named_parameters():
        assert torch.equal(p.detach().to(torch.bfloat16).float(), p.detach().float()), k


@pytest.mark.parametrize("size", R.SIZES)
def test_map_sizes(size):
    from sliders_conceptmod_amd import _native
    assert _native.lpips_map_sizes(*size) == R.MAP_SIZES[size]
    taps = R.reference("tiny_alex", size)[0]
    assert [tuple(t.shape[2:]) for t in taps] == R.MAP_SIZES[size]


@pytest.mark.parametrize("size", R.SIZES)
def test_reference_is_a_distance(size):
    a, b = R.pairs_u8(size)
    sd = R.weights("tiny_alex")
    xa, xb = R.to_input(a), R.to_input(b)
    d_ab = R.forward(sd, xa, xb)[2]
    assert torch.equal(R.forward(sd, xa, xa)[2], torch.zeros(len(R.AMPLITUDES), dtype=torch.float64))
    assert torch.allclose(R.forward(sd, xb, xa)[2], d_ab, rtol=1e-12, atol=0)
    assert (d_ab > 0).all()
    # the distances fall with the perturbation's amplitude
    assert all(d_ab[j] > d_ab[j + 1] for j in range(len(R.AMPLITUDES) - 1))


@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("net", R.NETS)
def test_every_mutation_clears_both_bars(net, size):
    """A condition on the inputs, not a measurement of the engine: a mistake in the metric must move the batch of
    distances by at least 3 x the wider (bf16) bar, or the GPU test could not tell it from rounding."""
    bar = max(R.bars(net, size, dt)["batch"] for dt in DTYPES)
    print(f"{net} {size}: batch bars fp16 {R.bars(net, size, DTYPES[0])['batch']:.3e} bf16 "
          f"{R.bars(net, size, DTYPES[1])['batch']:.3e}")
    for mutation in R.MUTATIONS:
        moved = R.mutated_batch_distance(net, size, mutation)
        print(f"  {mutation:<22} {moved:.3e} = {moved / bar:.1f} x the bar")
        assert moved > 3 * bar, (mutation, moved, bar)


def test_bars_come_from_the_twin_alone():
    for dt in DTYPES:
        b = R.bars("tiny_alex", (64, 64), dt)
        assert all(0 < v < 0.05 for v in b["taps"]) and 0 < b["batch"] < 0.01 and b["pair_abs"] > 0
    assert R.bars("tiny_alex", (64, 64), torch.float16)["batch"] < R.bars("tiny_alex", (64, 64), torch.bfloat16)["batch"]


# ---- host logic ----------------------------------------------------------------------------------------------------
def _write_tree(root):
    for folder in ("-1", "0", "half", "all", "2"):
        os.makedirs(os.path.join(root, folder))
    open(os.path.join(root, "lpips_score.csv"), "w").write("x\n")
    for name in ("4_0.png", "4_1.png", "14_0.png", "notes.txt", "9_0.png.bak"):
        open(os.path.join(root, "-1", name), "w").write("")


def test_folder_and_file_selection(tmp_path):
    from sliders_conceptmod_amd import lpips_score as S
    root = str(tmp_path)
    _write_tree(root)
    assert S.scale_folders(root, "0") == ["-1", "2", "half"]
    assert S.scale_folders(root, "2") == ["-1", "0", "half"]
    names = S.folder_files(os.path.join(root, "-1"))
    assert names == ["14_0.png", "4_0.png", "4_1.png", "9_0.png.bak"]  # names CONTAINING .png, as the script selects
    assert S.case_files(names, 4) == ["4_0.png", "4_1.png"]             # `14_0.png` does not start with `4_`
    assert S.case_files(names, 14) == ["14_0.png"] and S.case_files(names, 1) == []


def test_column_names():
    from sliders_conceptmod_amd import lpips_score as S
    assert [S.column_name(f) for f in ("-1", "half", "-half", "2")] == ["lpips_-1", "lpips_0.5", "lpips_-0.5", "lpips_2"]


@pytest.mark.parametrize("w,h", [(97, 61), (61, 97), (64, 64), (65, 64), (333, 127), (48, 40), (100, 31)])
def test_resize_geometry_against_pil(tmp_path, w, h):
    from PIL import Image
    from sliders_conceptmod_amd import lpips_score as S
    imsize = 37
    nw, nh = S.resized_size(w, h, imsize)
    assert min(nw, nh) == imsize and max(nw, nh) == int(imsize * max(w, h) / min(w, h))
    assert (nw <= nh) == (w <= h) or nw == nh
    u8 = np.random.RandomState(w * 1000 + h).randint(0, 256, (h, w, 3)).astype(np.uint8)
    path = str(tmp_path / "im.png")
    Image.fromarray(u8).save(path)
    got = S.load_rgb8(path, imsize)
    assert got.shape == (nh, nw, 3) and got.dtype == np.uint8
    want = np.asarray(Image.fromarray(u8).resize((nw, nh), resample=Image.BILINEAR))
    assert np.array_equal(got, want)
    assert S.resized_size(nw, nh, imsize) == (nw, nh)  # already at size: left alone
    assert np.array_equal(S.load_rgb8(path, min(w, h)), u8)


def test_load_rgb8_converts_to_rgb_and_names_an_unreadable_file(tmp_path):
    from PIL import Image
    from sliders_conceptmod_amd import lpips_score as S
    grey = str(tmp_path / "grey.png")
    Image.fromarray(np.arange(40 * 40, dtype=np.uint8).reshape(40, 40)).save(grey)
    assert S.load_rgb8(grey, 40).shape == (40, 40, 3)
    bad = str(tmp_path / "7_0.png")
    open(bad, "wb").write(b"not a png")
    with pytest.raises(RuntimeError, match="7_0.png"):
        S.load_rgb8(bad, 40)


def test_key_mapping_from_both_naming_schemes():
    from sliders_conceptmod_amd import lpips as PL, model_util
    src = model_util.load_lpips("synthetic://tiny_alex")
    ours = {k: v.clone() for k, v in src.state_dict().items()}
    assert set(ours) == ({f"{c}.{s}" for c in R.CONVS for s in ("weight", "bias")} |
                         {f"lin{i}.model.1.weight" for i in range(5)} | {"scaling_layer.shift", "scaling_layer.scale"})
    # torchvision's names (+ classifier keys, ignored) and the package's lin weights, in two steps
    tv = {}
    for idx, c in zip(PL.FEATURE_INDEX, R.CONVS):
        tv[f"features.{idx}.weight"], tv[f"features.{idx}.bias"] = ours[f"{c}.weight"], ours[f"{c}.bias"]
    tv["classifier.1.weight"], tv["classifier.1.bias"] = torch.zeros(8, 8), torch.zeros(8)
    lins = {k: v for k, v in ours.items() if k.startswith("lin")}
    m = PL.LPIPS(model_util.TINY_ALEX_CHANNELS)
    m.load_state_dict(tv, strict=False)
    m.load_state_dict(lins, strict=False)
    for k, v in ours.items():
        assert torch.equal(m.state_dict()[k], v), k
    # merged, strictly; the lin weights also as plain vectors
    m2 = PL.LPIPS(model_util.TINY_ALEX_CHANNELS)
    m2.load_state_dict({**tv, **{k: v.flatten() for k, v in lins.items()}}, strict=True)
    for k, v in ours.items():
        assert torch.equal(m2.state_dict()[k], v), k
    # a scaling layer that is not the metric's is refused
    with pytest.raises(Exception, match="scaling_layer.shift"):
        m2.load_state_dict({**ours, "scaling_layer.shift": torch.zeros(1, 3, 1, 1)})
    # the constants stay fp32 whatever the storage type
    m2 = m2.to(torch.bfloat16)
    assert m2.scaling_layer.scale.dtype == torch.float32 and m2.dtype == torch.bfloat16
    assert torch.equal(m2.scaling_layer.shift.flatten(), torch.tensor(PL.SHIFT))


@pytest.mark.parametrize("ext", ["safetensors", "pth"])
def test_load_lpips_from_a_directory_and_from_two_files(tmp_path, ext):
    from sliders_conceptmod_amd import lpips as PL, model_util
    src = model_util.load_lpips("synthetic://tiny_alex")
    sd = {k: v.detach().clone().contiguous() for k, v in src.state_dict().items()}
    tv = {}
    for idx, c in zip(PL.FEATURE_INDEX, R.CONVS):
        tv[f"features.{idx}.weight"], tv[f"features.{idx}.bias"] = sd[f"{c}.weight"], sd[f"{c}.bias"]
    tv["classifier.6.bias"] = torch.zeros(10)
    lins = {k: v for k, v in sd.items() if k.startswith("lin")}
    d = tmp_path / "w"
    d.mkdir()
    fa, fl = str(d / f"alexnet.{ext}"), str(d / f"alex_lin.{ext}")
    if ext == "safetensors":
        from safetensors.torch import save_file
        save_file(tv, fa)
        save_file(lins, fl)
    else:
        torch.save(tv, fa)
        torch.save(lins, fl)
    for name in (str(d), f"{fa},{fl}"):
        m = model_util.load_lpips(name)
        assert m.channels == model_util.TINY_ALEX_CHANNELS
        for k, v in sd.items():
            assert torch.equal(m.state_dict()[k], v), (name, k)
    with pytest.raises(ValueError, match="lin0.model.1.weight"):
        model_util.load_lpips(fa)  # the convolutions alone
    with pytest.raises(ValueError, match="net.slice1.0.weight"):
        model_util.load_lpips(fl)
    with pytest.raises(ValueError, match="synthetic://alex"):
        model_util.load_lpips(str(tmp_path / "nothing_here"))
    with pytest.raises(ValueError, match="synthetic://alex"):
        model_util.load_lpips("synthetic://vgg")


def test_pth_files_go_through_the_safe_unpickler(tmp_path):
    import pickle
    from sliders_conceptmod_amd import model_util

    class Boom:
        def __reduce__(self):
            return (os.system, ("true",))
    p = str(tmp_path / "evil.pth")
    torch.save({"lin0.model.1.weight": Boom()}, p)
    with pytest.raises(pickle.UnpicklingError):
        model_util.load_lpips(p)


def test_container_raises_on_the_cpu():
    from sliders_conceptmod_amd import _native, model_util
    m = model_util.load_lpips("synthetic://tiny_alex").half()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(_native.SmiError, match="no CPU fallback"):
        m(x, x)
    with pytest.raises(_native.SmiError, match="no CPU fallback"):
        m.distance(torch.zeros(1, 64, 64, 3, dtype=torch.uint8), torch.zeros(1, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(_native.SmiError, match="uint8"):
        m.distance(torch.zeros(1, 3, 64, 64, dtype=torch.uint8), torch.zeros(1, 3, 64, 64, dtype=torch.uint8))


def test_command_refuses_a_cpu_device(tmp_path):
    from sliders_conceptmod_amd import lpips_score
    with pytest.raises(ValueError, match="no CPU fallback"):
        lpips_score.main(["--im_path", str(tmp_path), "--prompts_path", str(tmp_path / "p.csv"), "--true", "0",
                          "--device", "cpu"])


def test_workspace_dry_run_and_refusals():
    """smi_lpips_workspace_bytes is a host-only dry run of the engine's graph; the refusals name their limit"""
    from sliders_conceptmod_amd import _native
    small = _native.lpips_workspace_bytes(R.ALEX, torch.float16, 1, 64, 64)
    large = _native.lpips_workspace_bytes(R.ALEX, torch.float16, 8, 64, 64)
    assert 2 * 2469696 <= small < large  # the packed filters alone are 2.47 M 16-bit values
    with pytest.raises(_native.SmiError, match="smaller than 31 x 31"):
        _native.lpips_workspace_bytes(R.ALEX, torch.float16, 1, 30, 30)
    with pytest.raises(_native.SmiError, match="smaller than 31 x 31"):
        _native.lpips_workspace_bytes(R.ALEX, torch.float16, 1, 64, 30)
    with pytest.raises(_native.SmiError, match=r"channels\[1\] = 20 must be a multiple of 8"):
        _native.lpips_workspace_bytes((16, 20, 32, 24, 16), torch.float16, 1, 64, 64)
    with pytest.raises(_native.SmiError, match="4 GiB"):
        _native.lpips_workspace_bytes(R.ALEX, torch.float16, 4096, 512, 512)
    for s in ("smi_lpips_workspace_bytes", "smi_lpips_create", "smi_lpips_distance"):
        assert s in _native.EXPORTED_SYMBOLS and hasattr(_native.lib(), s)


def test_score_sweep_on_a_stub_scorer(tmp_path):
    """the CSV logic with a scorer that needs no GPU: row-wise assignment, NaN for a case without files, `No File`"""
    pd = pytest.importorskip("pandas")
    from sliders_conceptmod_amd import lpips_score as S
    root = str(tmp_path)
    for folder, names in {"0": ["4_0.png", "9_0.png"], "half": ["4_0.png", "4_1.png", "9_0.png"], "all": ["4_0.png"]}.items():
        os.makedirs(os.path.join(root, folder))
        for n in names:
            open(os.path.join(root, folder, n), "w").write("")
    df = pd.DataFrame({"case_number": [9, 4, 6], "prompt": ["x", "y", "z"]})
    lines = []
    seen = []

    def scorer(pairs):
        seen.extend(pairs)
        return [float(len(os.path.basename(e))) + i for i, (o, e) in enumerate(pairs)]
    out = S.score_sweep(root, df, "0", scorer, log=lines.append)
    assert [c for c in out.columns if c.startswith("lpips_")] == ["lpips_0.5"]
    assert [os.path.basename(e) for _, e in seen] == ["9_0.png", "4_0.png"]  # 4_1.png has no original
    assert all(os.path.dirname(o).endswith("0") and os.path.dirname(e).endswith("half") for o, e in seen)
    assert lines.count("No File") == 1 and "Case 6: nan" in lines and "4_1.png" in lines
    assert out["lpips_0.5"].tolist()[:2] == [7.0, 8.0] and math.isnan(out["lpips_0.5"].tolist()[2])
    # a CSV of numbers only: the case numbers still select `4_...`, not `4.0_...`
    seen.clear()
    out = S.score_sweep(root, pd.DataFrame({"case_number": [4, 9], "evaluation_seed": [1.5, 2.5]}), "0", scorer,
                        log=lines.append)
    assert [os.path.basename(e) for _, e in seen] == ["4_0.png", "9_0.png"] and out["lpips_0.5"].notna().all()
