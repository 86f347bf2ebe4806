"""Host-side tests of the StyleMelGAN generator (a3t_amd/vocoder.py::StyleMelGANGeneratorHIP): the torch restatement
(tests/stylemelgan_ref.py) against the reference's outputs (tests/golden/stylemelgan.{npz,json}), its row rule, the noise-length
arithmetic, the packed operands, every refusal by field name, what a ragged batch hands its launches and SpeechEditor's
whole-utterance fallback.  No GPU."""
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stylemelgan_ref as R

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "stylemelgan.npz")), json.load(open(os.path.join(G, "stylemelgan.json")))


@pytest.fixture(scope="module")
def states():
    return {name: R.case_state(name) for name in R.CASES}


def _inputs(name, Tf, dseed=0):
    case = R.CASES[name]
    return (torch.from_numpy(R.mel_input(Tf, case["seed"], case["cfg"]["aux_channels"])),
            torch.from_numpy(R.noise_input(case["cfg"], Tf, case["seed"] + dseed)))


# ---------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_reproduces_the_reference(golden, states, name):
    arrays, meta = golden
    case, info = R.CASES[name], meta["cases"][name]
    assert info["cfg"] == case["cfg"] and info["seed"] == case["seed"] and info["gate_gain"] == case["gate_gain"]
    assert info["hop"] == R.hop_of(case["cfg"]) and info["noise_factor"] == R.noise_factor(case["cfg"])
    assert info["frames"] == list(case["frames"]) and (info["mel_seed"], info["noise_seed"]) == (1000 + case["seed"], 2000 + case["seed"])
    for Tf in case["frames"]:
        want = arrays[f"{name}.T{Tf}.wav64"]
        got = R.generator(states[name], case["cfg"], *_inputs(name, Tf), dtype=torch.float64).numpy()
        assert got.shape == want.shape == (Tf * info["hop"], 1)
        assert np.abs(got - want).max() <= 1e-9
        assert info["F"][str(Tf)] <= 2e-5 and all(0.02 <= v <= 20 for v in info["rms"][str(Tf)])
    assert info["noises_apart"] >= 0.1


def test_fixture_is_small(golden):
    assert sum(os.path.getsize(os.path.join(G, n)) for n in ("stylemelgan.npz", "stylemelgan.json")) < 512 * 1024


def test_rows_of_a_ragged_restatement_batch_are_the_rows_alone(states):
    name, lengths = "odd", (3, 13, 0, 7)
    cfg = R.CASES[name]["cfg"]
    Tm = max(lengths)
    c = torch.full((4, Tm, 80), float("nan"))
    z = torch.full((4, R.noise_steps(cfg, Tm), 32), float("nan"))
    rows = []
    for b, n in enumerate(lengths):
        mel, zb = _inputs(name, n, dseed=b)
        c[b, :n], z[b, :zb.shape[0]] = mel, zb
        rows.append((mel, zb))
    y = R.generator(states[name], cfg, c, z, lengths=lengths)
    hop = R.hop_of(cfg)
    assert y.shape == (4, Tm * hop, 1) and bool(torch.isfinite(y).all())
    for b, n in enumerate(lengths):
        if n:
            assert torch.equal(y[b, :n * hop], R.generator(states[name], cfg, *rows[b]))
        assert bool((y[b, n * hop:] == 0).all())
    blocks = []
    R.generator(states[name], cfg, *rows[1], blocks=blocks)
    assert [tuple(t.shape) for t in blocks[0]] == [(18, 64), (18, 80), (54, 64), (54, 64)] and len(blocks) == 3


# ----------------------------------------------------------------------------------------------------------- arithmetic
@pytest.mark.parametrize("name", list(R.CASES))
def test_noise_shape_and_network_length(states, name):
    from a3t_amd.vocoder import StyleMelGANGeneratorHIP
    cfg = R.CASES[name]["cfg"]
    gen = StyleMelGANGeneratorHIP(states[name], device="cpu", **cfg)
    Fn = int(np.prod(cfg["noise_upsample_scales"]))
    assert gen.noise_upsample_factor == Fn == R.noise_factor(cfg) and gen.hop == gen.upsample_factor == R.hop_of(cfg)
    assert gen.min_frames == 1 and gen.margin_frames is None
    for Tf, m in ((1, 1), (Fn - 1, 1), (Fn, 1), (Fn + 1, 2), (3 * Fn, 3)):
        assert gen.noise_shape(Tf) == (m, cfg["in_channels"]) == tuple(R.noise_input(cfg, Tf, 0).shape)
        assert R.n_eff(cfg, Tf) == m * Fn >= Tf > R.n_eff(cfg, Tf) - Fn
    if name == "v1_wn":
        assert (gen.hop, Fn) == (300, 80)


def test_defaults_are_the_24k_plan(states):
    from a3t_amd.vocoder import StyleMelGANGeneratorHIP
    gen = StyleMelGANGeneratorHIP(states["v1_wn"], device="cpu")
    assert (gen.hop, gen.noise_upsample_factor, gen.K, gen.dil, gen.Z, gen.A, gen.sigmoid) == (300, 80, 9, 2, 128, 80, False)
    assert gen.scales == (5, 1, 5, 1, 3, 1, 2, 2, 1) and gen.noise_scales == (10, 2, 2, 2) and gen.noise_slope == 0.2


# -------------------------------------------------------------------------------------------------------------- packers
def test_packed_operands(states):
    """Weight norm folded at load; every block convolution k-major [tap*Cin + in][out]; the transposed convolutions as 3-tap
    convolutions; the output convolution [K][C]."""
    from a3t_amd.vocoder import StyleMelGANGeneratorHIP, pack_hifigan_upsample
    st, cfg = states["v1_wn"], R.CASES["v1_wn"]["cfg"]
    w = R.folded(st, torch.float64)
    plain = {k: v.to(torch.float32).numpy() for k, v in w.items()}
    assert any(k.endswith("weight_v") for k in st) and not any(k.endswith("weight_v") for k in plain)
    a, b = StyleMelGANGeneratorHIP(st, device="cpu", **cfg), StyleMelGANGeneratorHIP(plain, device="cpu", **cfg)
    assert len(a.blocks) == 9 and [blk["u"] for blk in a.blocks] == cfg["upsample_scales"]
    names = dict(aux1="tade1.aux_conv.0", tade1="tade1.gated_conv.0", gate1="gated_conv1", aux2="tade2.aux_conv.0",
                 tade2="tade2.gated_conv.0", gate2="gated_conv2")
    for k, (ba, bb) in enumerate(zip(a.blocks, b.blocks)):
        for key, nm in names.items():
            wk, bk = ba[key]
            ref = w[f"blocks.{k}.{nm}.weight"].float()                      # [out][in][tap]
            cout, cin, taps = ref.shape
            assert torch.equal(wk, bb[key][0]) and tuple(wk.shape) == (taps * cin, cout) and wk.dtype == torch.float32
            assert torch.equal(wk.view(taps, cin, cout), ref.permute(2, 1, 0))
            assert torch.equal(bk, w[f"blocks.{k}.{nm}.bias"].float())
    assert tuple(a.blocks[0]["aux1"][0].shape) == (9 * 80, 64) and tuple(a.blocks[1]["aux1"][0].shape) == (9 * 64, 64)
    for i, (s, na) in enumerate(zip(cfg["noise_upsample_scales"], a.noise)):
        ref = w[f"noise_upsample.{2 * i}.weight"].float()                   # [in][out][2 s]
        assert torch.equal(na["w"], pack_hifigan_upsample(ref, s)) and tuple(na["w"].shape) == (s * 64, 3, ref.shape[0])
        assert torch.equal(na["b"], w[f"noise_upsample.{2 * i}.bias"].float().repeat(s))
    assert tuple(a.w_out.shape) == (9, 64) and torch.equal(a.w_out, w["output_conv.0.weight"].float()[0].t())
    nb = StyleMelGANGeneratorHIP(states["small_sigmoid"], device="cpu", **R.CASES["small_sigmoid"]["cfg"])
    assert nb.b_out is None and nb.blocks[0]["gate1"][1] is None and nb.noise[0]["b"] is None and nb.sigmoid
    with pytest.raises(ValueError, match="tade1.aux_conv.0"):
        StyleMelGANGeneratorHIP(st, device="cpu", **dict(cfg, kernel_size=7))


# ------------------------------------------------------------------------------------------------------------- refusals
V1_PARAMS = dict(in_channels=128, aux_channels=80, channels=64, out_channels=1, kernel_size=9, dilation=2, bias=True,
                 noise_upsample_scales=[10, 2, 2, 2], noise_upsample_activation="LeakyReLU",
                 noise_upsample_activation_params={"negative_slope": 0.2}, upsample_scales=[5, 1, 5, 1, 3, 1, 2, 2, 1],
                 upsample_mode="nearest", gated_function="softmax", use_weight_norm=True)


def test_from_config_builds_the_v1_plan(states):
    from a3t_amd.vocoder import StyleMelGANGeneratorHIP
    gen = StyleMelGANGeneratorHIP.from_config(states["v1_wn"], V1_PARAMS, device="cpu")
    ref = StyleMelGANGeneratorHIP(states["v1_wn"], device="cpu")
    assert gen.hop == 300 and gen.noise_slope == 0.2 and torch.equal(gen.blocks[8]["gate2"][0], ref.blocks[8]["gate2"][0])
    assert StyleMelGANGeneratorHIP.from_config(states["v1_wn"], dict(V1_PARAMS, noise_upsample_activation_params={}),
                                               device="cpu").noise_slope == 0.01


@pytest.mark.parametrize("change,field", [
    (dict(channels=32), "channels"), (dict(out_channels=4), "out_channels"), (dict(upsample_mode="linear"), "upsample_mode"),
    (dict(noise_upsample_activation="ReLU"), "noise_upsample_activation"), (dict(gated_function="tanh"), "gated_function"),
    (dict(kernel_size=8), "kernel_size"), (dict(kernel_size=11), "kernel_size"), (dict(in_channels=100), "in_channels"),
    (dict(aux_channels=40), "aux_channels"), (dict(noise_upsample_scales=[10, 1, 2, 2]), "noise_upsample_scales"),
    (dict(use_causal_conv=True), "use_causal_conv")])
def test_from_config_refuses_by_field_name(states, change, field):
    from a3t_amd.vocoder import StyleMelGANGeneratorHIP
    with pytest.raises(NotImplementedError, match=field):
        StyleMelGANGeneratorHIP.from_config(states["v1_wn"], dict(V1_PARAMS, **change), device="cpu")


def test_generator_types(states):
    from a3t_amd.vocoder import StyleMelGANGeneratorHIP, generator_from_config
    with pytest.raises(NotImplementedError, match="generator_type"):
        StyleMelGANGeneratorHIP.from_config(states["v1_wn"], V1_PARAMS, generator_type="MelGANGenerator", device="cpu")
    # the dispatch keeps its refusal in this change; its message names the class that does build the type
    with pytest.raises(NotImplementedError, match="generator_type.*StyleMelGANGeneratorHIP.from_config"):
        generator_from_config(states["v1_wn"], dict(generator_type="StyleMelGANGenerator", generator_params=V1_PARAMS), device="cpu")


def test_a_noise_of_the_wrong_shape_is_refused_before_any_launch(states):
    from a3t_amd.vocoder import StyleMelGANGeneratorHIP
    gen = StyleMelGANGeneratorHIP(states["odd"], device="cpu", **R.CASES["odd"]["cfg"])
    c = torch.zeros(13, 80)
    for z in (torch.zeros(2, 32), torch.zeros(3, 16), torch.zeros(13 * gen.hop, 1), torch.zeros(1, 3, 32)):
        with pytest.raises(ValueError, match=r"expected \(3, 32\)"):
            gen.inference(c, z)
    with pytest.raises(ValueError, match=r"expected \(2, 3, 32\)"):
        gen.inference(torch.zeros(2, 13, 80), torch.zeros(3, 32), lengths=(13, 2))
    with pytest.raises(ValueError, match="lengths"):
        gen.inference(torch.zeros(2, 13, 80), torch.zeros(2, 3, 32), lengths=(13, 14))
    with pytest.raises(ValueError, match="channels"):
        gen.inference(torch.zeros(13, 64), torch.zeros(3, 32))


def test_a_ragged_batch_goes_through_the_shared_preamble(states, monkeypatch):
    """What the launches of a ragged inference are given (every ops wrapper replaced by a recorder, so it runs without a GPU): the
    rows' lengths, their noise steps and, at every rate, the tile list of the rows' network lengths n_eff = ceil(L / F) * F;
    lengths are refused in prepare()'s words."""
    from a3t_amd import ops
    from a3t_amd.vocoder import StyleMelGANGeneratorHIP, pwg_tile_list
    cfg = R.ODD
    gen = StyleMelGANGeneratorHIP(states["odd"], device="cpu", **cfg)
    assert gen.noise_upsample_factor == 6 and gen.scales == (3, 2, 1)
    calls = []
    for name in ("zero_tail", "conv_fwd", "leaky_relu", "smg_stats", "smg_conv", "hfg_out"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append((_n, a, kw)))
    c, z = torch.randn(2, 9, 80), torch.randn(2, 2, 32)
    y = gen.inference(c, z, lengths=[9, 4])
    assert gen.hop == 6 and y.shape == (2, 9 * 6, 1)
    tails = [a for n, a, _ in calls if n == "zero_tail"]
    assert tails[0][1].tolist() == [2, 1] and tails[0][2:] == (1, 2, 2)             # the noise: 2 and 1 steps of the 2
    assert [t[1].tolist() for t in tails[1:3]] == [[2, 1]] * 2 and [t[2:] for t in tails[1:3]] == [(3, 2, 6), (6, 2, 12)]
    assert tails[-1][1].tolist() == [9, 4] and tails[-1][2:] == (6, 2, 12 * 6) and len(tails) == 4
    assert all(t[1].dtype == torch.int32 for t in tails)
    seen = {}
    for n, a, kw in calls:      # tiles of smg_conv (keyword; a = (x, w, b, y, B, T)), smg_stats (x, st, B, T, tiles), hfg_out
        tl, T = (kw["tiles"], a[5]) if n == "smg_conv" else (a[4], a[3]) if n == "smg_stats" else (a[7], a[5]) if n == "hfg_out" else (None, 0)
        if tl is not None:
            assert T % 12 == 0 and tl.dtype == torch.int32 and tl.is_contiguous() and tl.storage_offset() % 4 == 0
            assert tl.untyped_storage().data_ptr() == tails[-1][1].untyped_storage().data_ptr()      # one buffer, one copy
            seen.setdefault(T // 12, tl)
            assert tl is seen[T // 12]
    assert sorted(seen) == sorted(set(np.cumprod([1] + cfg["upsample_scales"]).tolist())) == [1, 3, 6]
    for rate, tl in seen.items():
        assert np.array_equal(tl.numpy(), pwg_tile_list([12, 6], rate))
    assert [n for n, _, _ in calls].count("smg_conv") == 18 and all(kw["tiles"] is not None for n, _, kw in calls if n == "smg_conv")
    hfg = [a for n, a, _ in calls if n == "hfg_out"]
    assert len(hfg) == 1 and hfg[0][7] is seen[6]
    # the refusals of the shared input check, in its words
    with pytest.raises(ValueError, match=re.escape("lengths= goes with a (B, Tmax, aux) batch")):
        gen.inference(c[0], z[0], lengths=[9])
    for bad in ([9], [9, 4, 1], [9, 10], [9, -1]):
        with pytest.raises(ValueError, match=re.escape(f"lengths {bad} do not fit a batch of 2 rows of 9 frames")):
            gen.inference(c, z, lengths=bad)
    # a dense batch packs nothing: no list, no tail to zero
    calls.clear()
    assert gen.inference(c, z).shape == (2, 9 * 6, 1)
    assert not [n for n, _, _ in calls if n == "zero_tail"]
    assert all(kw["tiles"] is None for n, _, kw in calls if n == "smg_conv")


# --------------------------------------------------------------------------------------------------------- SpeechEditor
class _FakeVocoder:
    """Records its calls; sample t of row b is c[b, t // hop, 0] + the row's first noise value."""
    hop = 300

    def __init__(self, margin_frames, shaped):
        self.margin_frames, self.calls = margin_frames, []
        if shaped:
            self.noise_shape = lambda frames: (-(-int(frames) // 80), 4)

    def inference(self, c, z=None, normalize_before=False, lengths=None):
        self.calls.append((tuple(c.shape), list(lengths), None if z is None else tuple(z.shape)))
        y = c[:, :, :1].repeat_interleave(self.hop, dim=1).clone()
        if z is not None:
            y = y + z.reshape(z.shape[0], -1)[:, :1, None]
        for b, n in enumerate(lengths):
            y[b, n * self.hop:] = 0
        return y


def _fake_editor(voc, flen=(90, 37), spans=((20, 30), (5, 9))):
    from a3t_amd.sedit import SpeechEditor
    ed = SpeechEditor.__new__(SpeechEditor)
    ed.vocoder, ed.hop, ed.fs, ed._loaded = voc, 300, 24000, None
    mel = torch.arange(2 * 96 * 3, dtype=torch.float32).reshape(2, 96, 3) / 100.0      # (padded beyond the longest row)
    plans = [SimpleNamespace(old_span_boundary=[s0, s1 - 2], new_span_boundary=[s0, s1]) for s0, s1 in spans]
    reqs = [SimpleNamespace(wav_org=np.full(n * 300 - 600, -1.0, dtype=np.float32)) for n in flen]
    ed._decode_batch = lambda requests: (plans, mel, None, list(flen))
    return ed, reqs, mel, plans


def test_speech_editor_vocodes_whole_utterances_without_a_margin():
    voc = _FakeVocoder(None, shaped=True)
    ed, reqs, mel, plans = _fake_editor(voc)
    z = [np.full((2, 4), 0.5, dtype=np.float32), np.full((1, 4), 0.25, dtype=np.float32)]
    span = ed.edit_batch(reqs, outputs=("orgin_replaced",), z=z)
    full = ed.edit_batch(reqs, z=z)
    assert voc.calls == [((2, 96, 3), [90, 37], (2, 2, 4))] * 2      # one ragged call over the whole utterances, z passed through
    for b, (s, f, p) in enumerate(zip(span, full, plans)):
        assert "prediction" not in s and f["prediction"].shape == ((90, 37)[b] * 300,)
        n0, n1 = p.new_span_boundary
        o0, o1 = (300 * x for x in p.old_span_boundary)
        want = np.concatenate([f["origin"][:o0], f["prediction"][300 * n0:300 * n1], f["origin"][o1:]])
        assert np.array_equal(s["orgin_replaced"], want) and np.array_equal(f["orgin_replaced"], want)
        assert float(f["prediction"][300 * n0]) == float(mel[b, n0, 0]) + (0.5, 0.25)[b]
    with pytest.raises(ValueError, match="noise_shape"):
        ed.edit_batch(reqs, z=[np.zeros((2, 4)), np.zeros((2, 4))])
    with pytest.raises(ValueError, match="noise_shape"):
        ed.edit_batch(reqs, z=[np.zeros(90 * 300), np.zeros(37 * 300)])
    assert ed.edit_batch(reqs, outputs=("orgin_replaced",))[0]["orgin_replaced"].shape == span[0]["orgin_replaced"].shape
    assert voc.calls[-1] == ((2, 96, 3), [90, 37], None)


def test_speech_editor_window_plan_is_unchanged_for_a_finite_margin():
    from a3t_amd.vocoder import span_window
    voc = _FakeVocoder(14, shaped=False)
    ed, reqs, mel, plans = _fake_editor(voc)
    span = ed.edit_batch(reqs, outputs=("orgin_replaced",))
    wins = [span_window(20, 30, 90, 14), span_window(5, 9, 37, 14)]
    assert wins == [(6, 44), (0, 23)]
    assert voc.calls == [((2, 38, 3), [38, 23], None)]
    for b, (s, p, (w0, w1)) in enumerate(zip(span, plans, wins)):
        n0, n1 = p.new_span_boundary
        assert float(s["orgin_replaced"][300 * p.old_span_boundary[0]]) == float(mel[b, n0, 0])
    z = [np.zeros(90 * 300, dtype=np.float32), np.zeros(37 * 300, dtype=np.float32)]
    ed.edit_batch(reqs, z=z)
    assert voc.calls[-1] == ((2, 96, 3), [90, 37], (2, 96 * 300, 1))
    with pytest.raises(ValueError, match="T_b \\* hop"):
        ed.edit_batch(reqs, z=[np.zeros((2, 4)), np.zeros((1, 4))])


def test_speech_editor_accepts_a_vocoder_without_a_margin():
    from a3t_amd.sedit import SpeechEditor

    class FE:
        fs, hop_length = 24000, 300

    class Model:
        feats_extract = FE()

    voc = _FakeVocoder(None, shaped=True)
    voc.min_frames = 1
    ed = SpeechEditor(Model(), None, voc, None, None)
    assert ed._ragged_vocoder()
