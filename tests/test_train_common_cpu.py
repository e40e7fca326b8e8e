"""The pure helpers of sliders_conceptmod_amd.train_common (no GPU, no native library): the fused-step rule, optimiser
argument parsing, command-line overrides, checkpoint cadence, the launch device and the trainers' parsers."""
import pytest
import torch

import sliders_conceptmod_amd.config_util as CU
from sliders_conceptmod_amd import train_common as TC
from sliders_conceptmod_amd import train_lora, train_lora_scale_xl, train_lora_xl


def _config(per_steps=2, iterations=6):
    return CU.RootConfig(
        prompts_file="unused", pretrained_model=CU.PretrainedModelConfig(name_or_path="synthetic://sd14"),
        network=CU.NetworkConfig(type="lierla", rank=8, alpha=4.0, training_method="noxattn"),
        train=CU.TrainConfig(precision="float16", noise_scheduler="ddim", iterations=iterations, lr=1e-4,
                             optimizer="AdamW", lr_scheduler="constant", max_denoising_steps=12),
        save=CU.SaveConfig(name="y", path="/models", per_steps=per_steps), logging=CU.LoggingConfig(),
        other=CU.OtherConfig())


@pytest.mark.parametrize("name, kwargs, fusable, weight_decay", [
    ("AdamW", {}, True, 1e-2),
    ("Adam", {}, True, 0),
    ("Adam", {"weight_decay": 0.1}, False, None),
    ("AdamW", {"amsgrad": True}, False, None),
    ("AdamW", {"foreach": False}, False, None),
    ("adamw", {"eps": 1e-3, "betas": (0.8, 0.9), "lr": 1e-4}, True, None),
    ("Lion", {}, False, None),
])
def test_adam_fusable(name, kwargs, fusable, weight_decay):
    got, wd = TC.adam_fusable(name, kwargs)
    assert got is fusable
    if weight_decay is not None:
        assert wd == weight_decay


def test_fused_step_choice():
    assert TC.fused_step_choice(None, "AdamW", {}) == (True, 1e-2)
    assert TC.fused_step_choice(True, "AdamW", {"weight_decay": 0.5}) == (True, 0.5)
    assert TC.fused_step_choice(False, "AdamW", {})[0] is False
    assert TC.fused_step_choice(None, "AdamW", {"foreach": False})[0] is False  # the autograd loop honours the argument
    with pytest.raises(ValueError, match="--fused_step implements Adam / AdamW"):
        TC.fused_step_choice(True, "AdamW", {"foreach": False})
    with pytest.raises(ValueError):
        TC.fused_step_choice(True, "Lion", {})


def test_parse_optimizer_args():
    assert TC.parse_optimizer_args(None) == {}
    assert TC.parse_optimizer_args("") == {}
    assert TC.parse_optimizer_args("eps=1e-3 betas=(0.8,0.9)") == {"eps": 1e-3, "betas": (0.8, 0.9)}


def test_apply_cli_overrides():
    config = _config()
    args = train_lora.build_parser().parse_args(["--alpha", "1.0", "--rank", "4", "--name", "x", "--attributes", "a, b"])
    assert TC.apply_cli_overrides(config, args) == ["a", "b"]
    assert config.save.name == "x_alpha1.0_rank4_noxattn"
    assert config.save.path.endswith("/x_alpha1.0_rank4_noxattn")
    assert (config.network.alpha, config.network.rank) == (1.0, 4)
    config = _config()
    assert TC.apply_cli_overrides(config, train_lora.build_parser().parse_args(["--alpha", "2"])) == []
    assert config.save.name == "y_alpha2.0_rank4_noxattn"  # no --name: the YAML's; --rank defaults to 4
    assert config.save.path == "/models/y_alpha2.0_rank4_noxattn"


def test_checkpoint_due():
    assert [i for i in range(6) if TC.checkpoint_due(i, _config(2, 6))] == [2, 4]
    assert [i for i in range(5) if TC.checkpoint_due(i, _config(2, 5))] == [2]  # the last step writes `_last` instead


def test_save_checkpoint(tmp_path):
    config = _config()
    config.save.path = str(tmp_path / "out" / "y")
    saved = []

    class Net:
        def save_weights(self, path, dtype=None):
            saved.append((path, dtype))

    TC.save_checkpoint(Net(), config, "4steps", ".safetensors", torch.float16)
    assert saved == [(tmp_path / "out" / "y" / "y_4steps.safetensors", torch.float16)]
    assert (tmp_path / "out" / "y").is_dir()


def test_launch_device(monkeypatch):
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    parser = train_lora.build_parser()
    with pytest.raises(ValueError, match="--device cpu"):
        TC.launch_device(parser.parse_args(["--alpha", "1", "--device", "cpu"]))
    assert TC.launch_device(parser.parse_args(["--alpha", "1", "--device", "3"])) == torch.device("cuda:3")
    assert TC.launch_device(parser.parse_args(["--alpha", "1"])) == torch.device("cuda:0")
    assert train_lora_scale_xl.launch_device is TC.launch_device  # the names the scripts had stay importable
    assert train_lora.add_fused_step_flags is TC.add_fused_step_flags


_TEXT_FLAGS = ["--config_file", "c.yaml", "--alpha", "1.5", "--rank", "8", "--device", "1", "--name", "n",
               "--attributes", "a, b"]


@pytest.mark.parametrize("module, extra", [
    (train_lora, []),
    (train_lora_xl, ["--peft_type", "dora"]),
    (train_lora_scale_xl, ["--folder_main", "d", "--stylecheck", "s", "--folders", "lo, hi", "--scales", "-1, 1"]),
])
def test_build_parsers_accept_the_full_flag_sets(module, extra):
    parser = module.build_parser()
    a = parser.parse_args(_TEXT_FLAGS + extra)
    assert (a.config_file, a.alpha, a.rank, a.device, a.name, a.attributes) == ("c.yaml", 1.5, 8, "1", "n", "a, b")
    assert (a.fused_step, a.no_dedup_uncond) == (None, False)
    assert parser.parse_args(_TEXT_FLAGS + extra + ["--fused_step"]).fused_step is True
    a = parser.parse_args(_TEXT_FLAGS + extra + ["--no_fused_step", "--no_dedup_uncond"])
    assert (a.fused_step, a.no_dedup_uncond) == (False, True)
    with pytest.raises(SystemExit):
        parser.parse_args(_TEXT_FLAGS + extra + ["--fused_step", "--no_fused_step"])
    if extra:
        for flag, value in zip(extra[::2], extra[1::2]):
            assert getattr(a, flag[2:]) == value
    d = module.build_parser().parse_args(["--alpha", "1"] + (["--folder_main", "d"] if module is train_lora_scale_xl else []))
    assert (d.rank, d.device, d.name, d.attributes) == (4, 0, None, None)
    assert d.config_file == ("data/config.yaml" if module is train_lora else "data/config-xl.yaml")
