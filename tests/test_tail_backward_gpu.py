"""smi_unet_backward_tail: the backward over the LAST n_live adapted samples of the saved pass, for callers whose output
gradient is exactly zero on the other adapted samples (the CFG-doubled adapted batch at guidance scale 1).

What is asserted, and where each bar comes from:

1. Under ONE pinned kernel selection (SMI_GEMM=128, SMI_GEMM_SPLITK=0, SMI_ATTN_BWD_FUSED=0: nothing may depend on the
   row count) the tail backward on d equals smi_unet_backward on [zeros ; d] BIT FOR BIT: per-sample arithmetic does not
   depend on the batch, a zero gradient row stays zero through every backward op, and the weight-gradient sums keep the
   full job's partition and order (the dead rows would add exact zeros).  LoRA, c3lier conv sites, per-sample
   multipliers; tiny SD-XL in fp16 / bf16 and the real SD-XL widths.
2. n_live == n_adapted is smi_unet_backward, bit for bit, at the default selection.
3. At the default selection the smaller row count may select other kernels (split-K slices, tuned tiles, the fused
   attention backward), so tail vs full agree to rounding only.  The bar is not a constant: it is 2 x the SELECTION NOISE of
   the full backward itself, measured in the same test as the distance between its gradient under the default and under
   the pinned selection (2 x: a GEMM change and an attention change can stack).  The tail gradient also has to meet the
   oracle bars of tests/test_engine_gpu.py unchanged (global 4.7e-3 fp16 / 3.7e-2 bf16).
4. SliderStep (batched, separate passes, dedup) and ImageSliderStep (one pass, one pass per side) at guidance 1 take the
   tail backward and agree with the same step forced onto the full backward: first loss bit-equal, weights after three
   steps within 2 x the selection noise of the full step's own weights; at guidance 3 the tail path is not taken.
5. Error paths: n_live out of range, no saved pass."""
import dataclasses
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as OU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = {"SMI_GEMM": "128", "SMI_GEMM_SPLITK": "0", "SMI_ATTN_BWD_FUSED": "0"}
CFGS = {"tiny_sdxl": OU.tiny_sdxl_config, "tiny_sd1x": OU.tiny_sd1x_config, "sdxl": OU.sdxl_config}


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def make_net(model, dtype, ou=None, c3lier=False, method="noxattn"):
    """Product UNet + LoRA network on the GPU; tiny models go through tests/test_engine_gpu.build_pair (so the oracle's
    adaptor of the same seeds has the same weights), the real widths are built here without an oracle adaptor."""
    if model != "sdxl":
        from tests.test_engine_gpu import build_pair
        ocfg, _ou, _onet, pu, pnet = build_pair(model, dtype, method=method, c3lier=c3lier)
        return ocfg, pu, pnet
    import sliders_conceptmod_amd.lora as L
    import sliders_conceptmod_amd.unet as PU
    ocfg = OU.sdxl_config()
    pu = PU.UNet2DConditionModel(PU.UNetConfig(**dataclasses.asdict(ocfg)))
    pu.load_state_dict(ou.state_dict())
    pu = pu.to("cuda", dtype).requires_grad_(False).eval()
    torch.manual_seed(1)
    pnet = L.LoRANetwork(pu, rank=4, multiplier=1.0, alpha=1.0, train_method=method)
    with torch.no_grad():
        pnet.flat_up.copy_(torch.randn(pnet.flat_up.shape, generator=torch.Generator().manual_seed(2)) * 0.02)
    pnet.to("cuda")
    return ocfg, pu, pnet


def live_gradient(n_live, hw):
    """d(loss)/d(eps) of the live samples: the size of d(MSE)/d(eps) at real shapes, another magnitude per sample (so that
    the per-sample power-of-two loss scales differ)."""
    d = torch.randn(n_live, 4, hw, hw, generator=torch.Generator().manual_seed(9)) * 1e-4
    for i in range(n_live):
        d[i] *= 3.0 ** i
    return d


def run_case(spec):
    """One saved forward per arm on the same inputs, then `full` = smi_unet_backward on [zeros ; d], `tail` =
    smi_unet_backward_tail on d, `tail_all` = the tail entry with n_live == n_adapted on [zeros ; d]."""
    from tests.test_engine_gpu import inputs, cuda_add
    out = {}
    ou = None
    if spec["model"] == "sdxl":
        torch.set_num_threads(16)
        ou = OU.init_synthetic_(OU.UNet2DConditionModel(OU.sdxl_config()), seed=0).requires_grad_(False).eval()
    n, na, nl, hw = spec["n"], spec["n_adapted"], spec["n_live"], spec["hw"]
    for dname in spec["dtypes"]:
        dtype = getattr(torch, dname)
        ocfg, pu, pnet = make_net(spec["model"], dtype, ou, spec.get("c3lier", False), spec.get("method", "noxattn"))
        x, ctx, add = inputs(ocfg, n, hw)
        cadd = cuda_add(add)
        te, ti = (cadd["text_embeds"].to(dtype).contiguous(), cadd["time_ids"].float().contiguous()) if cadd else (None, None)
        xc, cc = x.cuda().float().contiguous(), ctx.cuda().to(dtype).contiguous()
        flat, n_down, _ = pnet.engine_params()
        down, up = flat[:n_down], flat[n_down:]
        eng = pu._ensure_engine(n, hw, hw, 77, n_adapted=na)
        mult = spec.get("mults") or 1.0
        d = live_gradient(nl, hw).cuda()
        padded = torch.cat([torch.zeros(na - nl, 4, hw, hw, device="cuda"), d]).contiguous()
        for arm in spec["arms"]:
            eng.forward(xc, 499.0, cc, te, ti, down, up, mult, True, n_adapted=na)
            g = torch.zeros_like(flat)
            if arm == "full":
                eng.backward(padded, g[:n_down], g[n_down:])
            elif arm == "tail":
                eng.backward_tail(d, g[:n_down], g[n_down:])
            else:
                eng.backward_tail(padded, g[:n_down], g[n_down:])
            torch.cuda.synchronize()
            out[f"{dname}/{arm}"] = g.detach().cpu()
        out[f"{dname}/n_down"] = n_down
        pu._engine.close()
        del pu, pnet, eng
        torch.cuda.empty_cache()
    return out


def run_steps(spec):
    """Three steps of every step path at guidance 1 (and the guidance-3 routing check) with the tail backward on or forced
    off; returns first losses, all losses and the final weights per path, and which backward entry each path called."""
    import sliders_conceptmod_amd.lora as L
    import sliders_conceptmod_amd.model_util as MU
    import sliders_conceptmod_amd.unet as PU
    from sliders_conceptmod_amd import _native
    from sliders_conceptmod_amd.step import ImageSliderStep, SliderStep
    tail = spec["tail"]
    ocfg = OU.tiny_sdxl_config()
    ou = OU.init_synthetic_(OU.UNet2DConditionModel(ocfg), seed=0)
    calls = {"full": 0, "tail": 0}
    full0, tail0 = _native.Engine.backward, _native.Engine.backward_tail

    def full1(self, *a):
        calls["full"] += 1
        return full0(self, *a)

    def tail1(self, *a):
        calls["tail"] += 1
        return tail0(self, *a)

    _native.Engine.backward, _native.Engine.backward_tail = full1, tail1

    def fresh():
        pu = PU.UNet2DConditionModel(PU.UNetConfig(**dataclasses.asdict(ocfg)))
        pu.load_state_dict(ou.state_dict())
        pu = pu.to("cuda", torch.float16).requires_grad_(False).eval()
        torch.manual_seed(1)
        net = L.LoRANetwork(pu, rank=4, alpha=1.0, train_method="noxattn").to("cuda")
        with torch.no_grad():
            net.flat_up.copy_(torch.randn(net.flat_up.shape, generator=torch.Generator().manual_seed(2)) * 2e-2)
        sched = MU.create_noise_scheduler("euler_a")
        sched.set_timesteps(1000)
        return pu, net, sched

    g = torch.Generator().manual_seed(4)
    keys = ["target", "positive", "neutral", "unconditional"]
    emb = {k: torch.randn(1, 77, 64, generator=g) for k in keys}
    pooled = {k: torch.randn(1, 64, generator=g) for k in keys}
    tid = torch.tensor([[128.0, 128, 0, 0, 128, 128]])
    lat = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3)).cuda()
    out = {}
    text_paths = {"batched": {}, "separate": {"batch_passes": False}, "dedup": {"dedup_uncond": True}}
    for name, kw in list(text_paths.items()) + [("guidance3", {"cfg_scale": 3.0})]:
        pu, net, sched = fresh()
        t = sched.timesteps[400]
        step = SliderStep(pu, net, sched, lr=1e-3, weight_decay=1e-6, max_grad_norm=0.2, tail_backward=tail, **kw)
        cond = step.make_conditioning(emb, 2, pooled, tid)
        calls["full"] = calls["tail"] = 0
        losses = [float(step.train_step(lat, t, cond, "enhance", 2.0).item()) for _ in range(3)]
        out[name] = {"losses": losses, "weights": net.flat.detach().cpu().clone(), "calls": dict(calls)}
        pu._engine.close()
    g = torch.Generator().manual_seed(5)
    pe, ne, ue = (torch.randn(1, 77, 64, generator=g) for _ in range(3))
    pp, npool, up_ = (torch.randn(1, 64, generator=g) for _ in range(3))
    lo, hi, noise = (torch.randn(2, 4, 16, 16, generator=g) for _ in range(3))
    for name, one_pass, gs in (("image_one_pass", True, 1.0), ("image_two_pass", False, 1.0),
                               ("image_guidance3", True, 3.0), ("image_two_pass_guidance3", False, 3.0)):
        pu, net, sched = fresh()
        t = sched.timesteps[400]
        step = ImageSliderStep(pu, net, sched, lr=1e-3, weight_decay=1e-6, one_pass=one_pass, tail_backward=tail)
        cpos = step.make_conditioning(pe, 2, pp, tid, uncond=ue, uncond_pooled=up_)
        cneu = step.make_conditioning(ne, 2, npool, tid, uncond=ue, uncond_pooled=up_)
        calls["full"] = calls["tail"] = 0
        losses = []
        for _ in range(3):
            l = step.train_step(sched.add_noise(lo, noise, t).cuda(), sched.add_noise(hi, noise, t).cuda(), noise.cuda(),
                                noise.cuda(), t, cpos, cneu, 1.0, guidance_scale=gs)
            losses.append([float(v) for v in l.tolist()])
        out[name] = {"losses": losses, "weights": net.flat.detach().cpu().clone(), "calls": dict(calls)}
        pu._engine.close()
    return out


_CHILD = """
import json, sys, torch
root, fn, spec, out = sys.argv[1:5]
sys.path.insert(0, root)
import tests.test_tail_backward_gpu as T
torch.save(getattr(T, fn)(json.loads(spec)), out)
"""


def child(fn, spec, out, env=None):
    """Runs run_case / run_steps in a fresh process (the selection switches are read once per process)."""
    e = {k: v for k, v in os.environ.items() if k not in PINNED and k != "SMI_FULL_BACKWARD"}
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, fn, json.dumps(spec), str(out)], env=e, capture_output=True,
                       text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return torch.load(str(out), weights_only=False)


PINNED_CASES = {
    # frozen samples first (arow0 > 0), four adapted, the last two live
    "tiny_lora": {"model": "tiny_sdxl", "dtypes": ["float16", "bfloat16"], "n": 6, "n_adapted": 4, "n_live": 2, "hw": 16},
    "tiny_lora_full_xattn": {"model": "tiny_sdxl", "dtypes": ["float16", "bfloat16"], "method": "full", "n": 6,
                             "n_adapted": 4, "n_live": 2, "hw": 16},
    "tiny_sd1x_lora": {"model": "tiny_sd1x", "dtypes": ["float16"], "n": 4, "n_adapted": 4, "n_live": 2, "hw": 16},
    "tiny_c3lier": {"model": "tiny_sdxl", "dtypes": ["float16", "bfloat16"], "c3lier": True, "method": "full", "n": 6,
                    "n_adapted": 4, "n_live": 2, "hw": 16},
    "tiny_multipliers": {"model": "tiny_sdxl", "dtypes": ["float16", "bfloat16"], "n": 6, "n_adapted": 4, "n_live": 2,
                         "hw": 16, "mults": [1.5, -1.5, 0.75, -1.5]},
    "tiny_one_live_of_three": {"model": "tiny_sdxl", "dtypes": ["float16"], "n": 3, "n_adapted": 3, "n_live": 1, "hw": 16},
    "sdxl_real_widths": {"model": "sdxl", "dtypes": ["float16", "bfloat16"], "n": 3, "n_adapted": 2, "n_live": 1, "hw": 32},
}


@pytest.mark.parametrize("case", list(PINNED_CASES))
def test_tail_equals_full_on_zero_padded_gradient_bitwise_under_pinned_selection(case, tmp_path):
    spec = dict(PINNED_CASES[case], arms=["full", "tail"])
    res = child("run_case", spec, tmp_path / "r.pt", PINNED)
    for dname in spec["dtypes"]:
        full, tail, nd = res[f"{dname}/full"], res[f"{dname}/tail"], res[f"{dname}/n_down"]
        assert float(full[:nd].abs().max()) > 0 and float(full[nd:].abs().max()) > 0, "no gradient at all"
        print(f"{case} {dname}: tail vs full([zeros ; d]) rel diff down {rel(tail[:nd], full[:nd]):.2e}, "
              f"up {rel(tail[nd:], full[nd:]):.2e}")
        assert torch.equal(tail[:nd], full[:nd]), f"{case} {dname}: lora_down gradients differ"
        assert torch.equal(tail[nd:], full[nd:]), f"{case} {dname}: lora_up gradients differ"


@pytest.mark.parametrize("dname", ["float16", "bfloat16"])
def test_all_samples_live_is_the_full_backward_bitwise_at_default_selection(dname, tmp_path):
    spec = {"model": "tiny_sdxl", "dtypes": [dname], "n": 6, "n_adapted": 4, "n_live": 2, "hw": 16,
            "arms": ["full", "tail_all"]}
    res = child("run_case", spec, tmp_path / "r.pt")
    assert float(res[f"{dname}/full"].abs().max()) > 0
    assert torch.equal(res[f"{dname}/full"], res[f"{dname}/tail_all"])


def oracle_gradient(model, method, n, n_live, hw):
    """Flat fp32 LoRA gradient of the CPU oracle for the upstream gradient [zeros ; d] on an all-adapted batch."""
    from tests.test_engine_gpu import build_pair, inputs
    from oracle import slider_ref  # noqa: F401
    ocfg, ou, onet, pu, pnet = build_pair(model, torch.float16, method=method)
    x, ctx, add = inputs(ocfg, n, hw)
    gy = torch.cat([torch.zeros(n - n_live, 4, hw, hw), live_gradient(n_live, hw)])
    with onet:
        ref = ou(x, 499.0, ctx, add).sample
    (ref * gy).sum().backward()
    ref_flat = torch.zeros(pnet.flat.numel())
    n_down = pnet._n_down
    for lo, lp in zip(onet.unet_loras, pnet.unet_loras):
        gd, gu = lo.lora_down.weight.grad.flatten(), lo.lora_up.weight.grad.flatten()
        ref_flat[lp.off_down:lp.off_down + gd.numel()] = gd
        ref_flat[n_down + lp.off_up:n_down + lp.off_up + gu.numel()] = gu
    pu._engine and pu._engine.close()
    return ref_flat


SELECTION_CASES = {
    "tiny_sdxl": {"model": "tiny_sdxl", "dtypes": ["float16", "bfloat16"], "n": 4, "n_adapted": 4, "n_live": 2, "hw": 16},
    "sdxl_real_widths": {"model": "sdxl", "dtypes": ["float16"], "n": 2, "n_adapted": 2, "n_live": 1, "hw": 32},
}
ORACLE_BAR = {"float16": 4.7e-3, "bfloat16": 3.7e-2}  # tests/test_engine_gpu.py::test_lora_gradients_match_oracle, global


@pytest.mark.parametrize("case", list(SELECTION_CASES))
def test_tail_vs_full_at_default_selection_within_twice_the_selection_noise(case, tmp_path):
    """Measured (fp16 / bf16; DESIGN.md section 6 quotes them): see the printed line of each run."""
    spec = SELECTION_CASES[case]
    dflt = child("run_case", dict(spec, arms=["full", "tail"]), tmp_path / "d.pt")
    pinned = child("run_case", dict(spec, arms=["full"]), tmp_path / "p.pt", PINNED)
    ref = oracle_gradient(spec["model"], "noxattn", spec["n"], spec["n_live"], spec["hw"]) if case == "tiny_sdxl" else None
    for dname in spec["dtypes"]:
        full, tail, full_pinned = dflt[f"{dname}/full"], dflt[f"{dname}/tail"], pinned[f"{dname}/full"]
        noise = rel(full, full_pinned)  # what the parent's own arithmetic moves by when only the kernel selection changes
        diff = rel(tail, full)
        line = f"{case} {dname}: selection noise of the full backward {noise:.3e}, tail vs full {diff:.3e}"
        if ref is not None:
            e_tail, e_full = rel(tail, ref), rel(full, ref)
            line += f"; vs oracle: tail {e_tail:.3e}, full {e_full:.3e}"
        print(line)
        assert float(full.abs().max()) > 0
        assert diff <= 2.0 * noise, line
        if ref is not None:
            assert e_tail < ORACLE_BAR[dname], line


def test_steps_take_the_tail_backward_at_guidance_one_and_match_the_full_backward(tmp_path):
    tail = child("run_steps", {"tail": True}, tmp_path / "t.pt")
    full = child("run_steps", {"tail": False}, tmp_path / "f.pt")
    full_pinned = child("run_steps", {"tail": False}, tmp_path / "p.pt", PINNED)
    for name in ("batched", "separate", "dedup", "image_one_pass", "image_two_pass"):
        t, f, p = tail[name], full[name], full_pinned[name]
        assert t["calls"]["tail"] > 0 and t["calls"]["full"] == 0, (name, t["calls"])
        assert f["calls"]["tail"] == 0 and f["calls"]["full"] > 0, (name, f["calls"])
        noise = rel(f["weights"], p["weights"])
        diff = rel(t["weights"], f["weights"])
        print(f"{name}: weights after 3 steps, selection noise of the full step {noise:.3e}, tail vs full {diff:.3e}; "
              f"losses tail {t['losses']} full {f['losses']}")
        assert t["losses"][0] == f["losses"][0], (name, t["losses"], f["losses"])  # the forward is untouched
        assert diff <= 2.0 * noise, (name, diff, noise)
        for lt, lf in zip(t["losses"][1:], f["losses"][1:]):  # later losses see the weights: same bar, relative
            lt, lf = torch.tensor(lt, dtype=torch.float64), torch.tensor(lf, dtype=torch.float64)
            assert float((lt - lf).abs().max()) <= 2.0 * noise * float(lf.abs().max()), (name, t["losses"], f["losses"])
    for name in ("guidance3", "image_guidance3", "image_two_pass_guidance3"):  # guidance != 1: never the tail path
        assert tail[name]["calls"]["tail"] == 0 and tail[name]["calls"]["full"] > 0, (name, tail[name]["calls"])
        assert torch.equal(tail[name]["weights"], full[name]["weights"]), name


def test_error_paths():
    from sliders_conceptmod_amd import _native
    from tests.test_engine_gpu import build_pair, inputs, cuda_add
    dtype = torch.float16
    ocfg, ou, onet, pu, pnet = build_pair("tiny_sdxl", dtype)
    x, ctx, add = inputs(ocfg, 4, 16)
    cadd = cuda_add(add)
    te, ti = cadd["text_embeds"].half().contiguous(), cadd["time_ids"].float().contiguous()
    xc, cc = x.cuda().float().contiguous(), ctx.cuda().half().contiguous()
    flat, n_down, _ = pnet.engine_params()
    eng = pu._ensure_engine(4, 16, 16, 77, n_adapted=2)
    g = torch.zeros_like(flat)
    d = live_gradient(3, 16).cuda()
    with pytest.raises(_native.SmiError, match="no saved forward"):
        eng.backward_tail(d[:1].contiguous(), g[:n_down], g[n_down:])
    eng.forward(xc, 499.0, cc, te, ti, flat[:n_down], flat[n_down:], 1.0, True, n_adapted=2)
    with pytest.raises(_native.SmiError, match="live samples outside"):
        eng.backward_tail(d, g[:n_down], g[n_down:])  # 3 live of 2 adapted
    with pytest.raises(_native.SmiError, match="live samples outside"):
        _native.check(_native.lib().smi_unet_backward_tail(eng.handle, 0, _native.ptr(d), _native.ptr(g[:n_down]),
                                                           _native.ptr(g[n_down:])), "smi_unet_backward_tail")
    assert float(g.abs().max()) == 0.0
    eng.backward_tail(d[:1].contiguous(), g[:n_down], g[n_down:])  # the refused calls left the saved pass intact
    assert float(g.abs().max()) > 0.0
    with pytest.raises(_native.SmiError, match="no saved forward"):  # a backward consumes the saved pass
        eng.backward_tail(d[:1].contiguous(), g[:n_down], g[n_down:])


def test_dora_tail_backward_matches_the_oracle():
    """DoRA brings dY to ONE loss scale -- the minimum over the samples the backward runs on -- before the dense
    G = dY^T X.  A sample with a zero gradient reports scale 1, which usually was that minimum; the tail backward takes it
    over the live samples only, so its bits differ from the full backward's on [zeros ; d].  Both
    must meet the oracle bar of tests/test_engine_gpu.py::test_dora_forward_and_gradients_match_oracle (5.3e-3)."""
    import sliders_conceptmod_amd.dora as D
    import sliders_conceptmod_amd.unet as PU
    from oracle import slider_ref as R
    from tests.test_engine_gpu import inputs, cuda_add
    dtype = torch.float16
    ocfg = OU.tiny_sdxl_config()
    ou = OU.init_synthetic_(OU.UNet2DConditionModel(ocfg), seed=0).requires_grad_(False).eval()
    pu = PU.UNet2DConditionModel(PU.UNetConfig(**dataclasses.asdict(ocfg)))
    pu.load_state_dict(ou.state_dict())
    torch.manual_seed(1)
    onet = R.DoRANetworkRef(ou, 4, 1.0, 1.0, "noxattn")
    torch.manual_seed(1)
    pnet = D.DoRANetwork(pu, rank=4, multiplier=1.0, target_replace=["Attention"], train_method="noxattn")
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for lo, lp in zip(onet.unet_loras, pnet.unet_loras):
            w = torch.randn(lo.lora_up.weight.shape, generator=g) * 0.05
            sc = 1.0 + 0.1 * torch.randn(lo.dora_scale.shape, generator=g)
            lo.lora_up.weight.copy_(w)
            lp.lora_up.weight.copy_(w)
            lo.dora_scale.mul_(sc)
            lp.dora_scale.mul_(sc)
    pu = pu.to("cuda", dtype).requires_grad_(False).eval()
    pnet.to("cuda")
    n, nl, hw = 4, 2, 16
    x, ctx, add = inputs(ocfg, n, hw)
    d = live_gradient(nl, hw)
    gy = torch.cat([torch.zeros(n - nl, 4, hw, hw), d])
    with onet:
        ref = ou(x, 499.0, ctx, add).sample
    (ref * gy).sum().backward()
    cadd = cuda_add(add)
    te, ti = cadd["text_embeds"].half().contiguous(), cadd["time_ids"].float().contiguous()
    xc, cc = x.cuda().float().contiguous(), ctx.cuda().half().contiguous()
    flat, n_down, mult = pnet.engine_params()
    eng = pu._ensure_engine(n, hw, hw, 77)
    errs = {}
    for arm in ("full", "tail"):
        eng.forward(xc, 499.0, cc, te, ti, flat[:n_down], flat[n_down:], 1.0, True)
        gr = torch.zeros_like(flat)
        if arm == "full":
            eng.backward(gy.cuda().contiguous(), gr[:n_down], gr[n_down:])
        else:
            eng.backward_tail(d.cuda().contiguous(), gr[:n_down], gr[n_down:])
        pnet.flat.grad = gr
        for what in ("down", "up", "scale"):
            num = den = 0.0
            for lo, lp in zip(onet.unet_loras, pnet.unet_loras):
                a, b = {"down": (lp.lora_down.grad, lo.lora_down.weight.grad), "up": (lp.lora_up.grad, lo.lora_up.weight.grad),
                        "scale": (lp.dora_scale_grad, lo.dora_scale.grad)}[what]
                assert b is not None and float(b.abs().max()) > 0
                num += float((a.cpu() - b).norm() ** 2)
                den += float(b.norm() ** 2)
            errs[arm, what] = (num / den) ** 0.5
    print("dora vs oracle: " + ", ".join(f"{a} {w} {v:.2e}" for (a, w), v in errs.items()))
    assert all(v < 5.3e-3 for (a, _w), v in errs.items() if a == "tail"), errs
