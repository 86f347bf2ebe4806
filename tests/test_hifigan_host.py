"""Host-side checks of the HiFi-GAN generator (a3t_amd/vocoder.py::HiFiGANGeneratorHIP): the torch restatement
tests/hifigan_ref.py against the reference's own outputs (tests/golden/hifigan.{npz,json}, tests/golden/make_golden_hifigan.py),
weight-norm folding, the transposed convolution as a packed 3-tap convolution, the ragged rule and the span window of the
restatement, the margin formula, the refusals and the z argument.  No GPU.

Tolerance of every comparison against an fp64 result: hifigan_ref.bound = 4 x F, F the fp32-vs-fp64 loss of the reference on the
same input (from the fixture), floored at 1e-6 of scale."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hifigan_ref as R

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "hifigan.npz")), json.load(open(os.path.join(G, "hifigan.json")))


@pytest.fixture(scope="module")
def states():
    return {n: R.procedural_hifigan_state(c["cfg"], c["seed"], c["weight_norm"]) for n, c in R.CASES.items()}


NARROW = dict(R.V1, channels=64)      # the v1 plan's scales, kernels and dilations (so its margin) at an eighth of the width


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_against_the_reference(golden, states, name):
    arrays, meta = golden
    case, info = R.CASES[name], meta["cases"][name]
    assert info["cfg"] == case["cfg"] and info["seed"] == case["seed"] and meta["frames"] == list(R.FRAMES)
    for T in R.FRAMES:
        want = arrays[f"{name}.T{T}.wav64"]
        assert want.dtype == np.float64 and want.shape == (T * R.hop_of(case["cfg"]), 1)
        mel = torch.from_numpy(R.mel_input(T, case["seed"]))
        got64 = R.generator(states[name], case["cfg"], mel, dtype=torch.float64).numpy()
        assert np.abs(got64 - want).max() <= 1e-12
        got32 = R.generator(states[name], case["cfg"], mel, dtype=torch.float32).numpy().astype(np.float64)
        err = np.abs(got32 - want).max()
        print(name, T, "fp32 restatement vs fp64 reference", err, "bound", R.bound(info["F"][str(T)], R.scale_of(want)))
        assert err <= R.bound(info["F"][str(T)], R.scale_of(want))


def test_weight_normed_state_against_the_folded_state(states):
    from a3t_amd.vocoder import HiFiGANGeneratorHIP, fold_weight_norm
    cfg, st = R.V1, states["v1_wn"]
    plain = {k: v.to(torch.float32).numpy() for k, v in R.folded(st).items()}
    assert not any(k.endswith(("weight_g", "weight_v")) for k in plain) and any(k.endswith("weight_v") for k in st)
    for p, shp, _, _ in R.conv_names(cfg):
        v, g = torch.from_numpy(st[p + ".weight_v"]).double(), torch.from_numpy(st[p + ".weight_g"]).double()
        want = torch._weight_norm(v, g, 0)      # what torch.nn.utils.weight_norm computes, here in fp64
        got = fold_weight_norm(st, p)
        assert got.dtype == torch.float32 and tuple(got.shape) == shp
        assert (got.double() - want).abs().max() <= 2.0 ** -24 * want.abs().max()      # one fp32 rounding of the fp64 fold
        assert not torch.equal(got, torch.from_numpy(st[p + ".weight_v"]))
    kw = {k: v for k, v in cfg.items()}
    a = HiFiGANGeneratorHIP(st, device="cpu", fused=True, **kw)
    b = HiFiGANGeneratorHIP(plain, device="cpu", fused=True, **kw)
    assert torch.equal(a.w_in, b.w_in) and torch.equal(a.w_out, b.w_out)
    for sa, sb in zip(a.stages, b.stages):
        assert torch.equal(sa["w_up"], sb["w_up"]) and sa["fused"] == sb["fused"]
        for ba, bb in zip(sa["blocks"], sb["blocks"]):
            for ua, ub in zip(ba["units"], bb["units"]):
                assert all(torch.equal(x, y) for x, y in zip(ua["w"], ub["w"]))
    # the last two stages of the v1 plan (64 and 32 channels) are the fused kernel's, the wide ones run layer by layer
    assert [s["fused"] for s in a.stages] == [False, False, True, True] and a.fused_out and a.fused
    assert not HiFiGANGeneratorHIP(plain, device="cpu", fused=False, **kw).fused
    assert HiFiGANGeneratorHIP(plain, device="cpu", **kw).fused      # the default: the faster path (profiles/hifigan_latency.txt)


@pytest.mark.parametrize("s", [2, 3, 4, 5, 8])
def test_packed_upsample_is_the_transposed_convolution(s):
    from a3t_amd.vocoder import pack_hifigan_upsample
    g = torch.Generator().manual_seed(s)
    Cin, Cout, B, T = 6, 5, 2, 9
    w = torch.randn(Cin, Cout, 2 * s, generator=g, dtype=torch.float64)
    bias = torch.randn(Cout, generator=g, dtype=torch.float64)
    x = torch.randn(B, T, Cin, generator=g, dtype=torch.float64)
    want = F.conv_transpose1d(x.transpose(1, 2), w, bias, stride=s, padding=s // 2 + s % 2, output_padding=s % 2).transpose(1, 2)
    assert want.shape == (B, T * s, Cout)
    Wk = pack_hifigan_upsample(w, s)
    assert Wk.shape == (s * Cout, 3, Cin) and Wk.dtype == torch.float64
    # out[t][n] = bias[n] + sum_tap sum_c x[t + tap - 1][c] Wk[n][tap][c], zero padding: ops.conv_fwd(pad=1) spelled out
    xp = F.pad(x, (0, 0, 1, 1))
    got = sum(xp[:, tap:tap + T] @ Wk[:, tap].t() for tap in range(3)) + bias.repeat(s)
    got = got.reshape(B, T * s, Cout)       # [B*T][s*Cout] IS [B*T*s][Cout]
    assert (got - want).abs().max() <= 1e-12
    with pytest.raises(ValueError, match="kernel size"):
        pack_hifigan_upsample(w[:, :, :-1], s)


@pytest.mark.parametrize("plan", ["odd", "narrow_v1"])
def test_ragged_rows_of_the_restatement_are_the_rows_alone(states, plan):
    """Pins the restatement's ragged rule (tests/hifigan_ref.py), which the device tests compare against; it runs no product code.
    odd: no additional convolutions, no biases in the blocks; narrow_v1: the v1 plan at 64 channels, both of them."""
    cfg, st = (R.ODD, states["odd"]) if plan == "odd" else (NARROW, R.procedural_hifigan_state(NARROW, 7))
    lengths, hop = (13, 1, 7), R.hop_of(cfg)
    c = torch.full((3, 13, 80), float("nan"), dtype=torch.float64)
    for b, n in enumerate(lengths):
        c[b, :n] = torch.from_numpy(R.mel_input(n, 50 + b)).double()
    y = R.generator(st, cfg, c, lengths=lengths)
    assert y.shape == (3, 13 * hop, 1) and bool(torch.isfinite(y).all())
    for b, n in enumerate(lengths):
        alone = R.generator(st, cfg, c[b, :n])
        assert (y[b, :n * hop] - alone).abs().max() <= 1e-12
        assert bool((y[b, n * hop:] == 0).all())
    # the rule matters: without it the biases leak across the row's end
    loose = R.generator(st, cfg, torch.nan_to_num(c, nan=0.0))
    assert (loose[2, :7 * hop] - y[2, :7 * hop]).abs().max() > 1e-4


def test_margin_of_the_v1_plan():
    from a3t_amd.vocoder import HiFiGANGeneratorHIP, hifigan_margin_frames
    assert hifigan_margin_frames() in (19, 20)
    assert hifigan_margin_frames((5, 5, 4, 3), (3, 7, 11), ((1, 3, 5),) * 3, 7, True) == hifigan_margin_frames()
    # shorter reaches need less: no additional convolutions, smaller kernels
    assert hifigan_margin_frames(use_additional_convs=False) < hifigan_margin_frames()
    assert hifigan_margin_frames(resblock_kernel_sizes=(3, 5, 7)) < hifigan_margin_frames()
    st = R.procedural_hifigan_state(NARROW, 7)
    g = HiFiGANGeneratorHIP(st, device="cpu", **NARROW)
    assert g.margin_frames == hifigan_margin_frames() and g.upsample_factor == 300


def test_window_reproduces_the_span_with_the_margin_and_not_with_less():
    from a3t_amd.vocoder import hifigan_margin_frames
    st, hop, m = R.procedural_hifigan_state(NARROW, 7), 300, hifigan_margin_frames()
    c = torch.from_numpy(R.mel_input(60, 9)).double()
    full = R.generator(st, NARROW, c)
    n0, n1 = 25, 28

    def run(mel):
        return R.generator(st, NARROW, mel)

    inside = full[n0 * hop:n1 * hop]
    assert R.window(n0, n1, 60, m) == (n0 - m, n1 + m)      # the window is clipped at neither end: both margins are in play
    # "exactly": the same fp64 sums (the difference is 0.0 where this was written); 1e-13 is for torch builds whose convolution
    # blocks a sequence of another length differently
    assert (R.window_run(run, c, n0, n1, m, hop) - inside).abs().max() <= 1e-13
    # two frames less than the margin reach the span (about 1.4e-9 here: the outermost taps of five stages of small weights)
    assert (R.window_run(run, c, n0, n1, m - 2, hop) - inside).abs().max() > 1e-12
    # at the utterance's edges the window's edge is the utterance's edge
    assert (R.window_run(run, c, 0, 3, m, hop) - full[:3 * hop]).abs().max() <= 1e-13
    assert (R.window_run(run, c, 57, 60, m, hop) - full[57 * hop:]).abs().max() <= 1e-13


def _params(**kw):
    p = dict(in_channels=80, out_channels=1, channels=64, kernel_size=7, upsample_scales=[5, 5, 4, 3],
             upsample_kernel_sizes=[10, 10, 8, 6], resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5]] * 3,
             use_additional_convs=True, bias=True, nonlinear_activation="LeakyReLU",
             nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True)
    p.update(kw)
    return p


@pytest.mark.parametrize("kw,exc,field", [
    (dict(out_channels=4), NotImplementedError, "out_channels"),
    (dict(global_channels=256), NotImplementedError, "global_channels"),
    (dict(nonlinear_activation="ReLU", nonlinear_activation_params={}), NotImplementedError, "nonlinear_activation"),
    (dict(kernel_size=8), ValueError, "kernel_size"),
    (dict(resblock_kernel_sizes=[3, 6, 11]), ValueError, "resblock_kernel_sizes"),
    (dict(upsample_kernel_sizes=[10, 10, 8, 8]), ValueError, "upsample_kernel_sizes"),
    (dict(use_causal_conv=True), NotImplementedError, "use_causal_conv"),
])
def test_refusals_name_the_field(kw, exc, field):
    from a3t_amd.vocoder import HiFiGANGeneratorHIP
    st = R.procedural_hifigan_state(NARROW, 7)
    with pytest.raises(exc, match=field):
        HiFiGANGeneratorHIP.from_config(st, _params(**kw), device="cpu")


def test_config_loading_and_generator_type():
    from a3t_amd.vocoder import HiFiGANGeneratorHIP
    st = R.procedural_hifigan_state(NARROW, 7, weight_norm=True)
    g = HiFiGANGeneratorHIP.from_config(st, _params(), "HiFiGANGenerator", device="cpu")
    assert (g.scales, g.rk, g.K, g.add, g.slope, g.C0) == ((5, 5, 4, 3), (3, 7, 11), 7, True, 0.1, 64)
    # the zoo's older configs spell the key "upsample_kernal_sizes"
    p = _params()
    p["upsample_kernal_sizes"] = p.pop("upsample_kernel_sizes")
    assert HiFiGANGeneratorHIP.from_config(st, p, device="cpu").scales == (5, 5, 4, 3)
    for other in ("ParallelWaveGANGenerator", "MelGANGenerator", "StyleMelGANGenerator"):
        with pytest.raises(NotImplementedError, match="generator_type"):
            HiFiGANGeneratorHIP.from_config(st, _params(), other, device="cpu")
    with pytest.raises(NotImplementedError, match="shiny"):
        HiFiGANGeneratorHIP.from_config(st, _params(shiny=1), device="cpu")


def test_z_raises():
    from a3t_amd.vocoder import HiFiGANGeneratorHIP
    g = HiFiGANGeneratorHIP(R.procedural_hifigan_state(NARROW, 7), device="cpu", **NARROW)
    with pytest.raises(ValueError, match="z"):
        g.inference(torch.zeros(3, 80), z=torch.zeros(900, 1))
    with pytest.raises(ValueError, match="z"):
        g(torch.zeros(3, 80), torch.zeros(900, 1))


def test_pwg_refuses_another_channel_count():
    """The shared preamble refuses a c of the wrong width for ParallelWaveGAN too, before anything touches a device."""
    import pwg_f16_ref
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    g = ParallelWaveGANGeneratorHIP(pwg_f16_ref.vocoder_state(seed=4)[1], device="cpu")
    with pytest.raises(ValueError, match="79 channels"):
        g.inference(torch.zeros(5, 79))
    with pytest.raises(ValueError, match="goes with a"):
        g.inference(torch.zeros(5, 80), lengths=[5])
    with pytest.raises(ValueError, match="do not fit"):
        g.inference(torch.zeros(2, 5, 80), lengths=[5, 6])


@pytest.mark.parametrize("rates", [(300,), (25, 100, 300)])
def test_shared_preamble(rates):
    """prepare(): lens and one tile list per rate, all views of ONE int32 buffer, every list at a multiple of 4 words."""
    from a3t_amd.vocoder import HiFiGANGeneratorHIP, pwg_tile_list
    g = HiFiGANGeneratorHIP(R.procedural_hifigan_state(NARROW, 7), device="cpu", **NARROW)
    lengths, mel = (3, 0, 2), torch.randn(3, 3, 80, dtype=torch.float64)
    c, single, lens, tiles = g.prepare(mel, False, lengths, rates)
    assert c.dtype == torch.float32 and c.shape == (3, 3, 80) and torch.equal(c, mel.float()) and not single
    assert lens.dtype == torch.int32 and lens.tolist() == list(lengths) and lens.storage_offset() == 0
    assert list(tiles) == list(rates)
    end = 4      # lens [3], padded to 4 words
    for r in rates:
        want = pwg_tile_list(lengths, r)
        assert tiles[r].dtype == torch.int32 and tiles[r].is_contiguous() and np.array_equal(tiles[r].numpy(), want)
        assert tiles[r].untyped_storage().data_ptr() == lens.untyped_storage().data_ptr()
        assert tiles[r].storage_offset() % 4 == 0 and tiles[r].storage_offset() == end
        end += want.size
    assert lens.untyped_storage().nbytes() == 4 * end
    # without lengths: no buffer at all; a single utterance gains its batch dimension
    c1, single, lens, tiles = g.prepare(mel[0], False, None, rates)
    assert c1.shape == (1, 3, 80) and single and lens is None and tiles == {}
    with pytest.raises(ValueError, match="goes with a"):
        g.prepare(mel[0], False, [3], rates)
    with pytest.raises(ValueError, match="do not fit"):
        g.prepare(mel, False, (3, 4, 2), rates)
    with pytest.raises(ValueError, match="do not fit"):
        g.prepare(mel, False, (3, 2), rates)
