"""Host-side checks of the MelGAN / multi-band MelGAN generator (a3t_amd/vocoder.py::MelGANGeneratorHIP): the torch restatement
tests/melgan_ref.py against the reference's own outputs (tests/golden/melgan.{npz,json}, tests/golden/make_golden_melgan.py), the
numpy PQMF filter against the reference's, min_frames, the margin formula and the span window of the restatement, the packers,
the refusals of from_config / generator_from_config and the tile lists at the sub-band and full rates.  No GPU.

Tolerance of every comparison against an fp64 result: melgan_ref.bound = 4 x F, F the fp32-vs-fp64 loss of the reference on the
same input (from the fixture), floored at 1e-6 of scale."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import melgan_ref as R

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "melgan.npz")), json.load(open(os.path.join(G, "melgan.json")))


@pytest.fixture(scope="module")
def states():
    return {n: R.procedural_melgan_state(c["cfg"], c["seed"], c["weight_norm"]) for n, c in R.CASES.items()}


def _plan(cfg):
    return dict(upsample_scales=cfg["upsample_scales"], stacks=cfg["stacks"], stack_kernel_size=cfg["stack_kernel_size"],
                kernel_size=cfg["kernel_size"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_against_the_reference(golden, states, name):
    arrays, meta = golden
    case, info = R.CASES[name], meta["cases"][name]
    assert info["cfg"] == case["cfg"] and info["seed"] == case["seed"] and info["frames"] == list(case["frames"])
    assert info["pqmf"] == case["pqmf"]
    for T in case["frames"]:
        want = arrays[f"{name}.T{T}.wav64"]
        assert want.dtype == np.float64 and want.shape == (T * R.hop_of(case["cfg"]), 1)
        assert info["F"][str(T)] <= 1e-5      # the reference alone stays inside a tolerance worth testing
        mel = torch.from_numpy(R.mel_input(T, case["seed"]))
        got64 = R.generator(states[name], case["cfg"], mel, pqmf=case["pqmf"], dtype=torch.float64).numpy()
        assert np.abs(got64 - want).max() <= 1e-12
        got32 = R.generator(states[name], case["cfg"], mel, pqmf=case["pqmf"], dtype=torch.float32).numpy().astype(np.float64)
        err = np.abs(got32 - want).max()
        print(name, T, "fp32 restatement vs fp64 reference", err, "bound", R.bound(info["F"][str(T)], R.scale_of(want)))
        assert err <= R.bound(info["F"][str(T)], R.scale_of(want))


def test_ragged_rows_of_the_restatement_are_the_rows_alone(states):
    """Pins the restatement's ragged rule, which the device tests compare against: a row is the row alone whatever the padding
    holds, the output is zero behind it, and an empty row is all zeros.  The reflection itself as the index map of the rule."""
    case = R.CASES["odd"]
    cfg, st, hop = case["cfg"], states["odd"], R.hop_of(case["cfg"])
    lengths = (13, 4, 0, 5)
    c = torch.full((4, 13, 80), float("nan"), dtype=torch.float64)
    for b, n in enumerate(lengths):
        c[b, :n] = torch.from_numpy(R.mel_input(n, 50 + b)).double()
    y = R.generator(st, cfg, c, pqmf=case["pqmf"], lengths=lengths)
    assert y.shape == (4, 13 * hop, 1) and bool(torch.isfinite(y).all())
    for b, n in enumerate(lengths):
        if n:
            assert torch.equal(y[b, :n * hop], R.generator(st, cfg, c[b, :n], pqmf=case["pqmf"]))
        assert bool((y[b, n * hop:] == 0).all())
    # the rule matters: a row padded with zeros and run at full length is another signal
    loose = R.generator(st, cfg, torch.nan_to_num(c, nan=0.0), pqmf=case["pqmf"])
    assert (loose[3, :5 * hop] - y[3, :5 * hop]).abs().max() > 1e-4
    # a tap at ts < 0 reads -ts, one at ts >= W reads 2 (W - 1) - ts
    W, pad = 7, 5
    x = torch.arange(W, dtype=torch.float64)
    ts = torch.arange(-pad, W + pad)
    idx = torch.where(ts < 0, -ts, torch.where(ts >= W, 2 * (W - 1) - ts, ts))
    assert torch.equal(F.pad(x[None, None], (pad, pad), mode="reflect")[0, 0], x[idx])


def test_numpy_filter_is_the_reference_filter_bit_for_bit(golden):
    from a3t_amd.vocoder import pqmf_synthesis_filter
    arrays, _ = golden
    seen = 0
    for name, case in R.CASES.items():
        if case["pqmf"] is None:
            assert f"{name}.synthesis_filter" not in arrays
            continue
        want = arrays[f"{name}.synthesis_filter"]
        S = case["cfg"]["out_channels"]
        assert want.dtype == np.float32 and want.shape == (S, case["pqmf"]["taps"] + 1)
        got = pqmf_synthesis_filter(S, **case["pqmf"])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(R.pqmf_filter(S, **case["pqmf"]).view(np.uint32), want.view(np.uint32))
        seen += 1
    assert seen == 2
    with pytest.raises(ValueError):
        pqmf_synthesis_filter(4, taps=61)


def test_pqmf_formula_is_the_reference_chain():
    """y[n] = S sum_q sum_k h[k][S q - n + taps/2] x[q][k], the sum a3t_pqmf_synthesis computes, against the reference's
    conv_transpose1d + pad + conv1d in fp64."""
    for S, taps in ((4, 62), (4, 30), (3, 8)):
        h = R.pqmf_filter(S, taps, 0.15, 8.0)
        Ts = 23
        x = torch.randn(1, S, Ts, dtype=torch.float64, generator=torch.Generator().manual_seed(taps))
        want = R.pqmf_synthesis(x, h)[0, 0].numpy()
        got = np.zeros(Ts * S)
        for n in range(Ts * S):
            for q in range(Ts):
                i = S * q - n + taps // 2
                if 0 <= i <= taps:
                    got[n] += S * float(np.dot(h[:, i].astype(np.float64), x[0, :, q].numpy()))
        assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("name", list(R.CASES))
def test_min_frames(golden, states, name):
    from a3t_amd.vocoder import MelGANGeneratorHIP, melgan_min_frames
    case, info = R.CASES[name], golden[1]["cases"][name]
    assert melgan_min_frames(**_plan(case["cfg"])) == info["min_frames"] == min(case["frames"])
    gen = MelGANGeneratorHIP(states[name], device="cpu", pqmf=case["pqmf"], **case["cfg"])
    assert gen.min_frames == info["min_frames"] and gen.upsample_factor == info["hop"]
    # the restatement (torch's ReflectionPad1d rule) accepts it and rejects one less, like the reference
    mf = info["min_frames"]
    R.generator(states[name], case["cfg"], torch.zeros(mf, 80), pqmf=case["pqmf"], dtype=torch.float32)
    with pytest.raises(RuntimeError):
        R.generator(states[name], case["cfg"], torch.zeros(mf - 1, 80), pqmf=case["pqmf"], dtype=torch.float32)
    # refused on the host, before anything is launched (there is no device here)
    for bad in (dict(c=torch.zeros(mf - 1, 80)), dict(c=torch.zeros(2, mf + 3, 80), lengths=(mf + 3, mf - 1))):
        with pytest.raises(ValueError, match="min_frames"):
            gen.inference(**bad)
    with pytest.raises(ValueError, match="noise"):
        gen.inference(torch.zeros(mf, 80), z=torch.zeros(mf * info["hop"], 1))
    assert melgan_min_frames() == 6


def test_margin_of_the_v2_plan(states):
    """15 frames; on the fp64 restatement a window of that margin reproduces a span exactly, at mid-utterance and at both ends
    (where the window's reflection is the utterance's own), and one 3 frames narrower does not."""
    from a3t_amd.vocoder import MelGANGeneratorHIP, melgan_margin_frames, span_window
    case = R.CASES["mb_v2_wn"]
    cfg, st, hop = case["cfg"], states["mb_v2_wn"], 300
    assert melgan_margin_frames() == 15 == melgan_margin_frames(**_plan(cfg), out_channels=4, pqmf_taps=62)
    # plain_small by hand: 2 for the output convolution, + 4 -> ceil(6 / 2) + 1 = 4, + 4 -> ceil(8 / 4) + 1 = 3, + 2
    assert melgan_margin_frames([4, 2], 2, 3, 5, 1, 0) == 5
    gen = MelGANGeneratorHIP(st, device="cpu", **cfg)
    m = gen.margin_frames
    assert m == 15 and gen.upsample_factor == hop == R.hop_of(cfg) and m + 1 >= gen.min_frames
    T = 48
    c = torch.from_numpy(R.mel_input(T, 9)).double()

    def run(x):
        return R.generator(st, cfg, x, pqmf=case["pqmf"])

    full = run(c)
    scale = R.scale_of(full.numpy())
    for n0, n1 in ((20, 23), (0, 3), (45, 48), (3, 5)):
        w0, w1 = span_window(n0, n1, T, m)
        assert (w0, w1) == R.window(n0, n1, T, m)
        got = R.window_run(run, c, n0, n1, m, hop)
        assert float((got - full[n0 * hop:n1 * hop]).abs().max()) == 0.0, (n0, n1)
    narrow = R.window_run(run, c, 20, 23, m - 3, hop)
    assert float((narrow - full[20 * hop:23 * hop]).abs().max()) > 1e-3 * scale


def test_speech_editor_refuses_a_margin_below_min_frames():
    from a3t_amd.sedit import SpeechEditor

    class Voc:
        margin_frames, min_frames = 3, 6

        def inference(self, *a, **k):
            raise AssertionError

    class FE:
        fs, hop_length = 24000, 300

    class Model:
        feats_extract = FE()

    with pytest.raises(ValueError, match="min_frames"):
        SpeechEditor(Model(), None, Voc(), None, None)
    Voc.margin_frames = 5
    SpeechEditor(Model(), None, Voc(), None, None)


# ------------------------------------------------------------------------------------------------------------- packers
@pytest.mark.parametrize("C", [48, 96, 192, 16])
def test_packed_stack_is_the_residual_stack(C):
    """pack_melgan_stack spelled out in fp64: the rows of W1 | Ws | W2 (in the accumulator's order) and the two bias rows give
    the ResidualStack, the padding is zero."""
    from a3t_amd.vocoder import melgan_hidden_order, pack_melgan_stack
    g = torch.Generator().manual_seed(C)
    w1, w2, ws = (torch.randn(C, C, k, generator=g) for k in (3, 1, 1))
    b1, b2, bs = (torch.randn(C, generator=g) for _ in range(3))
    w, bias = pack_melgan_stack(w1, b1, w2, b2, ws, bs)
    Cp = (C + 31) // 32 * 32
    assert tuple(w.shape) == (4 * C + Cp, Cp) and tuple(bias.shape) == (2, Cp) and w.dtype == bias.dtype == torch.float32
    order = melgan_hidden_order(Cp)
    assert sorted(order.tolist()) == list(range(Cp))
    # register r of block j in lane half lk holds channel 32 j + (r & 3) + 8 (r >> 2) + 4 lk: rows 16 q + 2 kk + lk
    for q, kk, lk in ((0, 0, 0), (0, 0, 1), (0, 5, 1), (1, 0, 0), (Cp // 16 - 1, 7, 1)):
        r = 8 * (q & 1) + kk
        assert order[16 * q + 2 * kk + lk] == 32 * (q >> 1) + (r & 3) + 8 * (r >> 2) + 4 * lk
    assert bool((w[:, C:] == 0).all()) and bool((bias[:, C:] == 0).all())
    assert bool((w[4 * C:][torch.as_tensor(order) >= C] == 0).all())
    T, dil, slope = 40, 3, 0.2
    x = torch.randn(1, C, T, generator=g, dtype=torch.float64)
    h = F.conv1d(F.pad(F.leaky_relu(x, slope), (dil, dil), mode="reflect"), w1.double(), b1.double(), dilation=dil)
    want = F.conv1d(F.leaky_relu(h, slope), w2.double(), b2.double()) + F.conv1d(x, ws.double(), bs.double())
    wd, bd = w.double(), bias.double()
    a = F.pad(F.leaky_relu(x, slope), (dil, dil), mode="reflect")[0].t()                     # [T + 2 dil][C]
    hh = sum(a[tap * dil:tap * dil + T] @ wd[tap * C:(tap + 1) * C] for tap in range(3)) + bd[0]      # [T][Cp]
    hh = F.leaky_relu(hh, slope)
    got = x[0].t() @ wd[3 * C:4 * C] + hh[:, torch.as_tensor(order)] @ wd[4 * C:] + bd[1]
    assert (got[:, :C].t() - want[0]).abs().max() <= 1e-5 and bool((got[:, C:] == 0).all())      # (fp32 bias sum bs + b2)
    # without biases
    w0, bias0 = pack_melgan_stack(w1, None, w2, None, ws, None)
    assert torch.equal(w0, w) and bool((bias0 == 0).all())
    with pytest.raises(ValueError, match="ResidualStack"):
        pack_melgan_stack(torch.zeros(C, C, 5), None, w2, None, ws, None)


def test_weight_normed_state_and_the_width_dispatch(states):
    from a3t_amd.vocoder import MelGANGeneratorHIP
    case = R.CASES["mb_v2_wn"]
    st = states["mb_v2_wn"]
    plain = {k: v.to(torch.float32).numpy() for k, v in R.folded(st).items()}
    assert any(k.endswith("weight_v") for k in st) and not any(k.endswith("weight_v") for k in plain)
    a = MelGANGeneratorHIP(st, device="cpu", fused=True, **case["cfg"])
    b = MelGANGeneratorHIP(plain, device="cpu", fused=True, **case["cfg"])
    assert torch.equal(a.w_in, b.w_in) and torch.equal(a.w_out, b.w_out) and tuple(a.w_out.shape) == (4, 7, 48)
    for sa, sb in zip(a.stages, b.stages):
        assert torch.equal(sa["w_up"], sb["w_up"])
        assert all(torch.equal(ua["w"], ub["w"]) and torch.equal(ua["b"], ub["b"]) for ua, ub in zip(sa["stacks"], sb["stacks"]))
    assert [s["C"] for s in a.stages] == [192, 96, 48] and all(s["fused"] for s in a.stages) and a.fused_out and a.fused
    assert [u["dil"] for u in a.stages[0]["stacks"]] == [1, 3, 9, 27]
    assert tuple(a.h_syn.shape) == (4, 63)
    lay = MelGANGeneratorHIP(plain, device="cpu", fused=False, **case["cfg"])
    assert not lay.fused and not lay.fused_out and not any(s["fused"] for s in lay.stages)
    # the other plans: widths 32 / 16 run layer by layer, of 48 / 24 the first is built; the output convolution fits both
    small = MelGANGeneratorHIP(states["plain_small"], device="cpu", fused=True, **R.CASES["plain_small"]["cfg"])
    assert [s["fused"] for s in small.stages] == [False, False] and small.fused_out and small.pqmf is None
    assert small.upsample_factor == 8 and small.margin_frames == 5 and small.min_frames == 3
    odd = MelGANGeneratorHIP(states["odd"], device="cpu", fused=True, pqmf=R.CASES["odd"]["pqmf"], **R.CASES["odd"]["cfg"])
    assert [(s["C"], s["fused"]) for s in odd.stages] == [(48, True), (24, False)] and odd.fused_out
    assert odd.upsample_factor == 60 and tuple(odd.h_syn.shape) == (4, 31) and odd.b_in is None


# ------------------------------------------------------------------------------------------------------------ refusals
V2_PARAMS = dict(in_channels=80, out_channels=4, kernel_size=7, channels=384, upsample_scales=[5, 5, 3], stack_kernel_size=3,
                 stacks=4, use_weight_norm=True, use_causal_conv=False)


def test_from_config_builds_the_v2_plan(states):
    from a3t_amd.vocoder import MelGANGeneratorHIP, generator_from_config
    st = states["mb_v2_wn"]
    pq = dict(subbands=4, taps=62, cutoff_ratio=0.142, beta=9.0)
    gen = MelGANGeneratorHIP.from_config(st, V2_PARAMS, pqmf_params=pq, device="cpu")
    assert gen.slope == 0.2 and gen.final_tanh and gen.O == 4 and gen.scales == (5, 5, 3) and gen.upsample_factor == 300
    via = generator_from_config(st, dict(generator_type="MelGANGenerator", generator_params=V2_PARAMS, pqmf_params=pq), device="cpu",
                                fused=False)
    assert isinstance(via, MelGANGeneratorHIP) and not via.fused and torch.equal(via.w_in, gen.w_in)
    full = dict(V2_PARAMS, nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                pad="ReflectionPad1d", pad_params={}, use_final_nonlinear_activation=True, bias=True)
    assert MelGANGeneratorHIP.from_config(st, full, device="cpu").slope == 0.1


@pytest.mark.parametrize("change,field", [
    (dict(pad="ReplicationPad1d"), "pad"), (dict(pad_params={"value": 0.0}), "pad_params"),
    (dict(nonlinear_activation="ReLU"), "nonlinear_activation"), (dict(use_causal_conv=True), "use_causal_conv"),
    (dict(global_channels=8), "global_channels")])
def test_from_config_refuses_by_field_name(states, change, field):
    from a3t_amd.vocoder import MelGANGeneratorHIP, generator_from_config
    with pytest.raises(NotImplementedError, match=field):
        MelGANGeneratorHIP.from_config(states["mb_v2_wn"], dict(V2_PARAMS, **change), device="cpu")
    with pytest.raises(NotImplementedError, match=field):
        generator_from_config(states["mb_v2_wn"], dict(generator_type="MelGANGenerator", generator_params=dict(V2_PARAMS, **change)),
                              device="cpu")


def test_generator_types_and_pqmf_params(states):
    from a3t_amd.vocoder import HiFiGANGeneratorHIP, MelGANGeneratorHIP, generator_from_config
    st = states["mb_v2_wn"]
    with pytest.raises(NotImplementedError, match="generator_type"):
        MelGANGeneratorHIP.from_config(st, V2_PARAMS, generator_type="StyleMelGANGenerator", device="cpu")
    with pytest.raises(NotImplementedError, match="generator_type"):
        generator_from_config(st, dict(generator_type="StyleMelGANGenerator", generator_params={}), device="cpu")
    with pytest.raises(NotImplementedError, match="subbands"):
        MelGANGeneratorHIP.from_config(st, V2_PARAMS, pqmf_params=dict(subbands=8), device="cpu")
    with pytest.raises(NotImplementedError, match="window"):
        MelGANGeneratorHIP.from_config(st, V2_PARAMS, pqmf_params=dict(window="hann"), device="cpu")
    # HiFiGANGeneratorHIP.from_config keeps its behaviour and messages
    with pytest.raises(NotImplementedError, match="only HiFiGANGenerator is built here"):
        HiFiGANGeneratorHIP.from_config({}, {}, generator_type="MelGANGenerator")
    with pytest.raises(NotImplementedError, match="no multi-band / PQMF synthesis"):
        HiFiGANGeneratorHIP.from_config({}, dict(out_channels=4))
    with pytest.raises(NotImplementedError, match="no multi-band / PQMF synthesis"):
        generator_from_config({}, dict(generator_type="HiFiGANGenerator", generator_params=dict(out_channels=4)))


def test_generator_from_config_dispatches_to_the_other_two_families():
    import hifigan_ref as H
    from a3t_amd.vocoder import HiFiGANGeneratorHIP, ParallelWaveGANGeneratorHIP, generator_from_config
    case = H.CASES["odd"]
    hst = H.procedural_hifigan_state(case["cfg"], case["seed"], case["weight_norm"])
    params = {k: v for k, v in case["cfg"].items() if k != "negative_slope"}
    params.update(nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1})
    gen = generator_from_config(hst, dict(generator_type="HiFiGANGenerator", generator_params=params), device="cpu")
    assert isinstance(gen, HiFiGANGeneratorHIP) and gen.scales == (3, 2)
    # ParallelWaveGAN: a tiny plan, the constructor's arguments mapped and the rest refused by name
    L, Rc, Gc, Sc, A = 2, 4, 8, 4, 80
    from oracle.a3t_oracle import procedural_state
    shapes = {"first_conv.weight": (Rc, 1, 1), "first_conv.bias": (Rc,), "upsample_net.conv_in.weight": (A, A, 5),
              "last_conv_layers.1.weight": (Sc, Sc, 1), "last_conv_layers.1.bias": (Sc,), "last_conv_layers.3.weight": (1, Sc, 1),
              "last_conv_layers.3.bias": (1,)}
    for i, s in enumerate((2, 3)):
        shapes[f"upsample_net.upsample.up_layers.{2 * i + 1}.weight"] = (1, 1, 1, 2 * s + 1)
    for l in range(L):
        p = f"conv_layers.{l}."
        shapes.update({p + "conv.weight": (Gc, Rc, 3), p + "conv.bias": (Gc,), p + "conv1x1_aux.weight": (Gc, A, 1),
                       p + "conv1x1_out.weight": (Rc + Sc, Gc // 2, 1), p + "conv1x1_out.bias": (Rc + Sc,)})
    pst = procedural_state(shapes, 3)
    pp = dict(in_channels=1, out_channels=1, kernel_size=3, layers=L, stacks=1, residual_channels=Rc, gate_channels=Gc,
              skip_channels=Sc, aux_channels=A, aux_context_window=2, dropout=0.0, bias=True, use_weight_norm=True,
              use_causal_conv=False, upsample_conditional_features=True, upsample_net="ConvInUpsampleNetwork",
              upsample_params=dict(upsample_scales=[2, 3]))
    pwg = generator_from_config(pst, dict(generator_type="ParallelWaveGANGenerator", generator_params=pp), device="cpu")
    assert isinstance(pwg, ParallelWaveGANGeneratorHIP) and pwg.scales == (2, 3) and pwg.layers == L and not pwg.fused
    assert isinstance(generator_from_config(pst, dict(generator_params=pp), device="cpu"), ParallelWaveGANGeneratorHIP)
    for change, field in ((dict(kernel_size=5), "kernel_size"), (dict(use_causal_conv=True), "use_causal_conv"),
                          (dict(upsample_net="UpsampleNetwork"), "upsample_net"), (dict(out_channels=2), "out_channels"),
                          (dict(dropout=0.1), "dropout"), (dict(something_new=1), "something_new"),
                          (dict(upsample_params=dict(upsample_scales=[2, 3], freq_axis_kernel_size=3)), "freq_axis_kernel_size")):
        with pytest.raises(NotImplementedError, match=field):
            generator_from_config(pst, dict(generator_type="ParallelWaveGANGenerator", generator_params=dict(pp, **change)), device="cpu")


def test_tile_lists_at_the_sub_band_and_full_rates():
    """Multi-band v2: the last stage and the output convolution run at 75 samples per frame, the PQMF filter at 300; the lists
    of one batch (19, 0, 7 frames) at both rates, and prepare() hands out both."""
    from a3t_amd.vocoder import MelGANGeneratorHIP, pwg_tile_list
    lengths = (19, 0, 7)
    sub, full = pwg_tile_list(lengths, 75), pwg_tile_list(lengths, 300)
    assert sub.tolist() == [[0, 256 * i, 1425, 0] for i in range(6)] + [[2, 256 * i, 525, 0] for i in range(3)]
    assert full.tolist() == [[0, 256 * i, 5700, 0] for i in range(23)] + [[2, 256 * i, 2100, 0] for i in range(9)]
    assert all(int(w) % 4 == 0 for w in full[:, 2])      # a row's full-rate length is a multiple of the sub-band count
    case = R.CASES["mb_v2_wn"]
    gen = MelGANGeneratorHIP(R.procedural_melgan_state(case["cfg"], 1, False), device="cpu", **case["cfg"])
    c, single, lens, tiles = gen.prepare(torch.zeros(3, 19, 80), False, lengths, (5, 25, 75, 300))
    assert not single and lens.tolist() == list(lengths) and sorted(tiles) == [5, 25, 75, 300]
    assert np.array_equal(tiles[75].numpy(), sub) and np.array_equal(tiles[300].numpy(), full)
