"""`python -m sliders_conceptmod_amd.lpips_score` on synthetic://tiny_alex: the CSV it writes against the API."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IMSIZE = 40


def _write_sweep(root):
    """folders -1, 0 (true), half, all and a .csv entry; two image sizes; 4_1.png of `-1` has no original"""
    from PIL import Image
    rs = np.random.RandomState(11)
    files = {"0": ["4_0.png", "9_0.png", "9_1.png"], "-1": ["4_0.png", "4_1.png", "9_0.png", "9_1.png"],
             "half": ["4_0.png", "9_0.png"], "all": ["4_0.png"]}
    sizes = {"4_0.png": (48, 40), "4_1.png": (48, 40), "9_0.png": (50, 80), "9_1.png": (48, 40)}  # (w, h)
    base = {name: rs.randint(0, 256, (h, w, 3)).astype(np.int64) for name, (w, h) in sizes.items()}
    for folder, names in files.items():
        os.makedirs(os.path.join(root, folder))
        for name in names:
            im = base[name] if folder == "0" else np.clip(base[name] + rs.randint(-40, 41, base[name].shape), 0, 255)
            Image.fromarray(im.astype(np.uint8)).save(os.path.join(root, folder, name))
    open(os.path.join(root, "old_scores.csv"), "w").write("case_number\n")
    return files


def _run(root, csv, bs, dtype="fp16"):
    from sliders_conceptmod_amd import lpips_score
    lpips_score.main(["--im_path", root, "--prompts_path", csv, "--true", "0", "--lpips_model", "synthetic://tiny_alex",
                      "--imsize", str(IMSIZE), "--batch_size", str(bs), "--dtype", dtype])
    return open(os.path.join(root, "lpips_score.csv"), "rb").read()


def test_lpips_score_command(tmp_path, capsys):
    pd = pytest.importorskip("pandas")
    from sliders_conceptmod_amd import lpips_score, model_util
    csv = str(tmp_path / "prompts.csv")
    # the index differs from the case numbers; case 6 has no images
    pd.DataFrame({"case_number": [9, 4, 6], "prompt": ["x", "y", "z"], "evaluation_seed": [1, 2, 3]}).to_csv(csv, index=False)
    outputs = []
    for bs in (1, 4):
        root = str(tmp_path / f"images_bs{bs}")
        files = _write_sweep(root)
        outputs.append(_run(root, csv, bs))
    assert outputs[0] == outputs[1]  # the batch size never changes a CSV
    printed = capsys.readouterr().out
    assert printed.count("No File") == 2 and "Case 6: nan" in printed  # 4_1.png of `-1`, once per run
    df = pd.read_csv(os.path.join(root, "lpips_score.csv"))
    assert [c for c in df.columns if c.startswith("lpips_")] == ["lpips_-1", "lpips_0.5"]
    assert list(df.case_number) == [9, 4, 6] and list(df.prompt) == ["x", "y", "z"]
    # every value recomputed through the API, one pair at a time
    model = model_util.load_lpips("synthetic://tiny_alex").to("cuda", torch.float16)
    for folder, col in (("-1", "lpips_-1"), ("half", "lpips_0.5")):
        for case in (9, 4):
            vals = []
            for name in files[folder]:
                if name.startswith(f"{case}_") and name in files["0"]:
                    a = lpips_score.load_rgb8(os.path.join(root, "0", name), IMSIZE)
                    b = lpips_score.load_rgb8(os.path.join(root, folder, name), IMSIZE)
                    assert min(a.shape[:2]) == IMSIZE
                    vals.append(float(model.distance(torch.from_numpy(a.copy())[None], torch.from_numpy(b.copy())[None])[0]))
            assert vals and all(v > 0 for v in vals)
            got = float(df[df.case_number == case].iloc[0][col])
            assert got == pytest.approx(float(np.mean(vals)), rel=1e-12), (folder, case)
        assert math.isnan(float(df[df.case_number == 6].iloc[0][col]))
    assert df["lpips_-1"].notna().sum() == 2 and df["lpips_-1"].std() > 0


def test_unreadable_png_raises_with_its_name(tmp_path):
    pd = pytest.importorskip("pandas")
    csv = str(tmp_path / "prompts.csv")
    pd.DataFrame({"case_number": [4, 9]}).to_csv(csv, index=False)
    root = str(tmp_path / "images")
    _write_sweep(root)
    open(os.path.join(root, "half", "9_0.png"), "wb").write(b"\x89PNG\r\n\x1a\n truncated")
    with pytest.raises(RuntimeError, match="9_0.png"):
        _run(root, csv, 4)


def test_pair_of_two_sizes_raises_with_both_names(tmp_path):
    pd = pytest.importorskip("pandas")
    from PIL import Image
    csv = str(tmp_path / "prompts.csv")
    pd.DataFrame({"case_number": [4]}).to_csv(csv, index=False)
    root = str(tmp_path / "images")
    _write_sweep(root)
    Image.fromarray(np.zeros((40, 60, 3), dtype=np.uint8)).save(os.path.join(root, "half", "4_0.png"))
    with pytest.raises(RuntimeError, match=r"0.4_0\.png.*half.4_0\.png"):
        _run(root, csv, 4)
