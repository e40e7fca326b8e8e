"""The restated flow-matching Euler scheduler (model_util.FlowMatchEulerDiscreteScheduler) and the SD3 step helpers of
train_util, without a GPU: the schedule's documented properties, the package's scheduler against the restatement of
tests/mmdit_refs.py, and the loop's bookkeeping on a stand-in transformer."""
import pytest
import torch

import mmdit_refs as R
from sliders_conceptmod_amd import model_util as MU
from sliders_conceptmod_amd import train_util as TU


def test_schedule_properties():
    s = MU.FlowMatchEulerDiscreteScheduler()
    assert s.num_train_timesteps == 1000 and s.shift == 3.0 and s.init_noise_sigma == 1.0
    assert float(s.shift_sigma(torch.tensor(0.5, dtype=torch.float64))) == 0.75
    s.set_timesteps(28)
    assert len(s.timesteps) == 28 and len(s.sigmas) == 29
    assert float(s.timesteps[0]) == 1000.0 and float(s.sigmas[0]) == 1.0 and float(s.sigmas[-1]) == 0.0
    assert bool((s.sigmas[1:] < s.sigmas[:-1]).all()) and bool((s.timesteps[1:] < s.timesteps[:-1]).all())
    x = torch.randn(2, 3)
    assert s.scale_model_input(x, s.timesteps[3]) is x


@pytest.mark.parametrize("n", [1 + 3, 28, 50])
def test_schedule_matches_the_restatement(n):
    s = MU.FlowMatchEulerDiscreteScheduler()
    s.set_timesteps(n)
    ts, sig = R.flow_sigmas(n)
    assert torch.equal(s.timesteps, ts.float()) and torch.equal(s.sigmas, sig.float())
    # shifted TWICE: once for the training sigmas whose ends span the linspace, once more on the inference grid
    once = torch.linspace(float(R.shift_sigma(torch.tensor(1.0))), float(R.shift_sigma(torch.tensor(1e-3))), n,
                          dtype=torch.float64)
    assert not torch.allclose(sig[:-1], once) and torch.allclose(sig[:-1], R.shift_sigma(once))


def test_constant_velocity_integrates_to_x0_minus_sigma0_v():
    s = MU.FlowMatchEulerDiscreteScheduler()
    s.set_timesteps(28)
    g = torch.Generator().manual_seed(0)
    x0, v = torch.randn(2, 16, 4, 4, generator=g), torch.randn(2, 16, 4, 4, generator=g)
    x = x0
    for t in s.timesteps:
        x = s.step(v, t, x).prev_sample
    want = x0 - float(s.sigmas[0]) * v
    assert x.dtype == torch.float32 and float((x - want).abs().max()) <= 28 * 2 ** -23 * float(want.abs().max() + v.abs().max())


class _Stand:
    """A transformer stand-in: records its calls, returns a velocity that depends on the timestep."""

    def __init__(self):
        self.calls = []

    def __call__(self, hidden_states, timestep, encoder_hidden_states, pooled_projections, multipliers=None,
                 return_dict=True):
        self.calls.append((list(timestep), tuple(hidden_states.shape), multipliers))
        return (hidden_states * 0 + torch.tensor(timestep).reshape(-1, 1, 1, 1) / 1000.0,)


def test_predict_noise_sd3_returns_the_stepped_latents_and_feeds_1000_sigma():
    s = MU.FlowMatchEulerDiscreteScheduler()
    s.set_timesteps(4)
    tr = _Stand()
    lat = torch.ones(2, 16, 2, 2)
    te, pooled = torch.zeros(4, 5, 8), torch.zeros(4, 8)
    t = s.timesteps[1]
    out = TU.predict_noise_sd3(tr, s, t, lat, te, pooled, guidance_scale=3.0)
    ts, shape, _m = tr.calls[0]
    assert shape == (4, 16, 2, 2) and ts == [float(t)] * 4
    assert abs(float(t) - 1000.0 * float(s.sigmas[1])) <= 2 ** -23 * 1000.0  # both stored in fp32
    v = float(t) / 1000.0  # u == c: guidance changes nothing
    want = lat + (float(s.sigmas[2]) - float(s.sigmas[1])) * v
    assert torch.allclose(out, want, atol=1e-6) and not torch.allclose(out, torch.full_like(out, v))


def test_diffusion_sd3_runs_exactly_the_slice():
    s = MU.FlowMatchEulerDiscreteScheduler()
    s.set_timesteps(6)
    tr = _Stand()
    lat = torch.zeros(1, 16, 2, 2)
    TU.diffusion_sd3(tr, s, lat, torch.zeros(2, 5, 8), torch.zeros(2, 8), guidance_scale=1.0, total_timesteps=5,
                     start_timesteps=2)
    assert [c[0][0] for c in tr.calls] == [float(t) for t in s.timesteps[2:5]]


def test_restated_loop_agrees_with_the_package_loop_on_a_linear_model():
    s = MU.FlowMatchEulerDiscreteScheduler()
    s.set_timesteps(4)
    lat = torch.randn(2, 16, 2, 2, generator=torch.Generator().manual_seed(1))

    def fn(x2, t):
        return 0.3 * x2 + t / 1000.0

    class Lin:
        def __call__(self, hidden_states, timestep, **_):
            return (fn(hidden_states.double(), timestep[0]).float(),)
    got = TU.diffusion_sd3(Lin(), s, lat, None, None, guidance_scale=2.0)
    want = R.sweep_loop(fn, lat, 4, 2.0)
    assert float((got.double() - want).abs().max()) < 1e-5


def test_initial_latents_and_concat():
    s = MU.FlowMatchEulerDiscreteScheduler()
    lat = TU.get_initial_latents_sd3(s, 3, 64, 48, 2, generator=torch.manual_seed(4))
    assert tuple(lat.shape) == (3, 16, 8, 6)
    u, c = torch.zeros(1, 4, 8), torch.ones(1, 4, 8)
    e = TU.concat_embeddings_sd3(u, c, 2)
    assert tuple(e.shape) == (4, 4, 8) and float(e[:2].sum()) == 0 and float(e[2:].min()) == 1
