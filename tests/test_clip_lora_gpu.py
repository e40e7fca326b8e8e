"""The differentiable CLIP text tower (smi_clip_lora_*: LoRA on self_attn.{q,k,v}_proj and out_proj, one multiplier per
sample, a saved pass and its backward) on a tiny tower -- hidden 128, 2 heads, 2 layers, intermediate 256, 77 positions,
rank 4, lora_up seeded non-zero -- against torch autograd through the float64 tower of tests/notrigger_refs.py.

Bar: relative L2 against the exact reference A at most 3 e_q + 1e-4, e_q being the distance from A of the same reference
with every stored tensor (values and gradients) rounded to the engine's dtype; over the whole gradient and per site.
tests/test_notrigger_refs_cpu.py shows that a dropped site, a flipped multiplier and a dropped layer miss it."""
import pytest
import torch

import notrigger_refs as R

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
RANK, ALPHA, MULTS = 4, 1.0, [1.0, -1.0]
WHICH = ["last_layer_out", "penultimate"]


class Setup:
    """The tiny tower, its LoRA and the gradient that enters the backward: built once, shared, never modified."""

    def __init__(self):
        self.cfg = R.tiny_config()
        self.sd32 = R.tiny_state(self.cfg)
        self.sd = {k: v.double() for k, v in self.sd32.items()}
        self.ids = R.tiny_ids(self.cfg, 2)
        self.names = R.site_names(self.cfg.num_hidden_layers)
        g = torch.Generator().manual_seed(11)
        self.lora = R.make_lora(self.names, self.cfg.hidden_size, RANK, ALPHA, g)
        self.d_hidden = torch.randn((2, 77, self.cfg.hidden_size), generator=g, dtype=torch.float64).float()
        self.sites, self.n_down, self.n_up = R.flat_layout(self.names, self.cfg.hidden_size, RANK, ALPHA)
        self.down, self.up = R.flatten_lora(self.lora, self.names)
        self._refs = {}

    def ref(self, which, dtype=None):
        """(d_down, d_up) float64 of the two-sample pass; dtype None: exact (A), else storage-rounded (B)."""
        if (which, dtype) not in self._refs:
            self._refs[(which, dtype)] = R.tower_grads(self.sd, self.ids, self.cfg.num_attention_heads, self.cfg.hidden_act,
                                                       self.lora, self.names, MULTS, ALPHA / RANK, self.d_hidden.double(),
                                                       which, dtype)
        return self._refs[(which, dtype)]

    def engine(self, dt, batch=2, sites=None):
        from sliders_conceptmod_amd import _native
        state = {k: v.to(dt).cuda().contiguous() for k, v in self.sd32.items()}
        return _native.ClipLoraEngine(self.cfg, dt, state, self.sites if sites is None else sites, batch, torch.device("cuda"))


@pytest.fixture(scope="module")
def S():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return Setup()


def eos_of(S, ids):
    return (ids == S.cfg.eos_token_id).int().argmax(dim=-1)


def grads_of(S, eng, which, samples=slice(None), mults=MULTS, between=None):
    """One saved forward and its backward; returns (d_down, d_up) fp32 on the CPU and the forward's outputs."""
    ids = S.ids[samples]
    down, up = S.down.cuda(), S.up.cuda()
    out = eng.forward_lora(ids, eos_of(S, ids), down, up, mults, save=True)
    if between is not None:
        between()
    dd, du = torch.zeros(S.n_down, device="cuda"), torch.zeros(S.n_up, device="cuda")
    eng.backward(S.d_hidden[samples].contiguous().cuda(), dd, du, which=WHICH.index(which))
    torch.cuda.synchronize()
    return dd.cpu(), du.cpu(), out


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("dt", DT, ids=["fp16", "bf16"])
def test_lora_gradients_against_f64_autograd(S, dt, which):
    eng = S.engine(dt)
    dd, du, out = grads_of(S, eng, which)
    A, B = torch.cat(S.ref(which)), torch.cat(S.ref(which, dt))
    got = torch.cat([dd, du]).double()
    assert torch.isfinite(got).all()
    e_q, e = R.rel(B, A), R.rel(got, A)
    print(f"{which} {dt}: whole gradient e {e:.3e}  e_q {e_q:.3e}  ratio {e / e_q:.2f}")
    assert e <= R.bar(e_q), (e, e_q)
    d, r = S.cfg.hidden_size, RANK
    worst = 0.0
    for i, nm in enumerate(S.names):  # per site: down block i of the first flat vector, up block i of the second
        for part, (g, a, b) in (("down", (dd, S.ref(which)[0], S.ref(which, dt)[0])), ("up", (du, S.ref(which)[1], S.ref(which, dt)[1]))):
            sl = slice(i * r * d, (i + 1) * r * d)
            if float(a[sl].abs().max()) == 0.0:  # penultimate: the last layer's sites get a zero gradient
                assert which == "penultimate" and ".layers.1." in nm and float(g[sl].abs().max()) == 0.0, (nm, part)
                continue
            eq_s, e_s = R.rel(b[sl], a[sl]), R.rel(g[sl], a[sl])
            worst = max(worst, e_s / eq_s)
            assert e_s <= R.bar(eq_s), (nm, part, e_s, eq_s)
    print(f"{which} {dt}: worst per-site ratio e / e_q {worst:.2f}")
    # the forward's outputs against the float64 tower under the same adaptor
    ref = R.tower_forward(S.sd, S.ids, S.cfg.num_attention_heads, S.cfg.hidden_act, S.lora, MULTS, ALPHA / RANK)
    refq = R.tower_forward(S.sd, S.ids, S.cfg.num_attention_heads, S.cfg.hidden_act, S.lora, MULTS, ALPHA / RANK, dt)
    for k_out, k_ref in (("last_layer_out", "last_layer_out"), ("penultimate", "penultimate"), ("last_hidden", "last_hidden_state")):
        assert R.rel(out[k_out], ref[k_ref]) <= R.bar(R.rel(refq[k_ref], ref[k_ref])), k_out
    # and the adaptor matters: the frozen tower is outside that bar (8 % away, against bars of 0.2 % / 1.5 %)
    frozen = R.tower_forward(S.sd, S.ids, S.cfg.num_attention_heads, S.cfg.hidden_act)
    assert R.rel(frozen["last_layer_out"], ref["last_layer_out"]) > 2 * R.bar(R.rel(refq["last_layer_out"], ref["last_layer_out"]))
    eng.close()


@pytest.mark.parametrize("dt", DT, ids=["fp16", "bf16"])
def test_one_pass_of_two_samples_equals_two_passes_of_one(S, dt):
    eng = S.engine(dt)
    dd, du, out = grads_of(S, eng, "last_layer_out")
    parts = [grads_of(S, eng, "last_layer_out", slice(i, i + 1), MULTS[i:i + 1]) for i in range(2)]
    both = torch.cat([dd, du]).double()
    summed = torch.cat([parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]]).double()
    e_q = R.rel(torch.cat(S.ref("last_layer_out", dt)), torch.cat(S.ref("last_layer_out")))
    e = R.rel(both, summed)
    print(f"{dt}: two samples in one pass against two passes {e:.3e} (bar {R.bar(e_q):.3e})")
    assert e <= R.bar(e_q)
    # the forward of each sample: bit for bit what a one-sample pass through the same per-sample route gives
    for i in range(2):
        for k in out:
            assert torch.equal(out[k][i:i + 1].view(torch.int16), parts[i][2][k].view(torch.int16)), (i, k)
    eng.close()


@pytest.mark.parametrize("dt", DT, ids=["fp16", "bf16"])
def test_zero_multipliers_and_encode_give_the_frozen_bits(S, dt):
    from sliders_conceptmod_amd import _native
    eng = S.engine(dt)
    state = {k: v.to(dt).cuda().contiguous() for k, v in S.sd32.items()}
    frozen = _native.ClipEngine(S.cfg, dt, state, 2, torch.device("cuda"))
    eos = eos_of(S, S.ids)
    want = frozen.encode(S.ids, eos)
    got = eng.encode(S.ids, eos)  # smi_clip_encode on the LoRA engine
    zero = eng.forward_lora(S.ids, eos, S.down.cuda(), S.up.cuda(), [0.0, 0.0])
    torch.cuda.synchronize()
    for w, g, z in zip(want, got, (zero["last_hidden"], zero["penultimate"], zero["pooled"])):
        assert torch.equal(w.view(torch.int16), g.view(torch.int16)) and torch.equal(w.view(torch.int16), z.view(torch.int16))
    on = eng.forward_lora(S.ids, eos, S.down.cuda(), S.up.cuda(), MULTS)
    assert not torch.equal(on["last_hidden"].view(torch.int16), want[0].view(torch.int16))
    eng.close()
    frozen.close()


def test_no_grad_calls_between_forward_and_backward_change_nothing(S):
    dt = torch.float16
    eng = S.engine(dt)
    dd, du, _ = grads_of(S, eng, "last_layer_out")
    eos = eos_of(S, S.ids)
    other_down = (S.down * 0.5).cuda()

    state = {k: v.to(dt).cuda().contiguous() for k, v in S.sd32.items()}
    from sliders_conceptmod_amd import _native
    frozen = _native.ClipEngine(S.cfg, dt, state, 2, torch.device("cuda"))
    want = frozen.encode(S.ids, eos)

    def between():  # a frozen encode, then an adapted no-grad pass with other parameters and other multipliers
        got = eng.encode(S.ids, eos)  # on the engine that holds a saved adapted pass: still the frozen tower's bits
        assert all(torch.equal(g.view(torch.int16), w.view(torch.int16)) for g, w in zip(got, want))
        eng.forward_lora(S.ids, eos, other_down, S.up.cuda(), [0.3, 2.0])

    dd2, du2, _ = grads_of(S, eng, "last_layer_out", between=between)
    assert torch.equal(dd, dd2) and torch.equal(du, du2)
    frozen.close()
    # a backward consumes the saved pass: a second one is refused
    with pytest.raises(_native.SmiError, match="no saved forward"):
        eng.backward(S.d_hidden.cuda(), torch.zeros(S.n_down, device="cuda"), torch.zeros(S.n_up, device="cuda"))
    eng.close()


def test_refusals_leave_the_engine_working(S):
    from sliders_conceptmod_amd import _native
    dt = torch.float16
    with pytest.raises(_native.SmiError, match="DoRA"):
        S.engine(dt, sites=[dict(s, off_dora=i * S.cfg.hidden_size) for i, s in enumerate(S.sites)])
    eng = S.engine(dt, batch=2)
    ids3 = R.tiny_ids(S.cfg, 3)
    with pytest.raises(_native.SmiError, match="batch 3"):
        eng.forward_lora(ids3, eos_of(S, ids3), S.down.cuda(), S.up.cuda(), [1.0, 1.0, 1.0])
    dd, du, _ = grads_of(S, eng, "last_layer_out")
    assert R.rel(torch.cat([dd, du]), torch.cat(S.ref("last_layer_out"))) < 5e-3
    eng.close()
