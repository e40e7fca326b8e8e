"""`python -m sliders_conceptmod_amd.clip_score` on synthetic://tiny_clip: the CSV it writes against the API."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PROMPT = "a photo of an old person"


def _write_sweep(root):
    from PIL import Image
    rs = np.random.RandomState(7)
    files = {"-1": ["4_0.png", "4_1.png", "9_0.png"], "0": ["4_0.png", "9_0.png", "9_1.png"], "half": ["4_0.png", "9_0.png"],
             "all": ["4_0.png"]}
    k = 0
    for folder, names in files.items():
        os.makedirs(os.path.join(root, folder))
        for name in names:
            w, h = ((48, 40), (40, 48))[k % 2]
            k += 1
            Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, folder, name))
    return files


def test_clip_score_command(tmp_path):
    pd = pytest.importorskip("pandas")
    from PIL import Image
    from sliders_conceptmod_amd import clip_score, model_util
    from sliders_conceptmod_amd.clip import clip_image_preprocess
    csv = str(tmp_path / "prompts.csv")
    # the index differs from the case numbers; case 6 has no images
    pd.DataFrame({"case_number": [9, 4, 6], "prompt": ["x", "y", "z"], "evaluation_seed": [1, 2, 3]}).to_csv(csv, index=False)
    outputs = []
    for bs in (1, 4):
        root = str(tmp_path / f"images_bs{bs}")
        files = _write_sweep(root)
        clip_score.main(["--im_path", root, "--prompt", f" {PROMPT} ", "--prompts_path", csv, "--clip_model",
                         "synthetic://tiny_clip", "--batch_size", str(bs), "--dtype", "fp16"])
        outputs.append(open(os.path.join(root, "clip_scores.csv"), "rb").read())
    assert outputs[0] == outputs[1]  # the batch size never changes a CSV
    df = pd.read_csv(os.path.join(root, "clip_scores.csv"))
    assert [c for c in df.columns if c.startswith("clip_")] == ["clip_-1", "clip_0", "clip_0.5"]
    assert list(df.case_number) == [9, 4, 6]
    # every value recomputed through the API
    model, tok, size = model_util.load_clip("synthetic://tiny_clip")
    model = model.to("cuda", torch.float16)
    te = model.get_text_features(tok([PROMPT]).input_ids.cuda())
    for folder, col in (("-1", "clip_-1"), ("0", "clip_0"), ("half", "clip_0.5")):
        for case in (9, 4):
            vals = []
            for name in files[folder]:
                if name.startswith(f"{case}_"):
                    u8 = clip_image_preprocess(Image.open(os.path.join(root, folder, name)), size)
                    emb = model.get_image_features(rgb8=torch.from_numpy(u8.copy())[None].cuda())
                    vals.append(float(model.logits(emb, te)[0, 0]))
            got = float(df[df.case_number == case].iloc[0][col])
            assert got == pytest.approx(float(np.mean(vals)), rel=1e-12), (folder, case)
        assert math.isnan(float(df[df.case_number == 6].iloc[0][col]))
    assert df["clip_-1"].notna().sum() == 2 and df["clip_-1"].std() > 0
