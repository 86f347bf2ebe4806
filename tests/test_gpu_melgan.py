"""MelGAN / multi-band MelGAN generator on the device (a3t_amd/vocoder.py::MelGANGeneratorHIP, csrc/melgan.hip): the four kernels
against fp64 torch, the whole generator layer by layer and fused against the reference's outputs (tests/golden/melgan.{npz,json}),
ragged batches, span windows and SpeechEditor with this vocoder.

Tolerance of every numeric comparison (the rule of test_gpu_hifigan.py::_check): the yardstick is the fp64 result, the bound 4 x F
(melgan_ref.bound), where F is what an fp32 evaluation by the reference (fixture cases) or by torch on the CPU (kernel cases,
computed here) loses against fp64 on the same input, floored at 1e-6 of scale: both sides are fp32 evaluations of the same sums in
different orders.  Measured device values: profiles/melgan_parity.txt."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import melgan_ref as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
B, T = 2, 300      # one full tile and a partial one
SENTINEL = 7.5
SLOPE = 0.2


def _tiles(lengths, rate=1):
    from a3t_amd.vocoder import pwg_tile_list
    return torch.from_numpy(pwg_tile_list(lengths, rate)).to(DEV)


def _check(what, got, ref64, ref32, scale=None):
    """got (device fp32) against ref64 within 4 x F, F from ref32 (the CPU's fp32 evaluation)."""
    scale = float(ref64.abs().max()) if scale is None else scale
    Fl = float((ref32.double() - ref64).abs().max()) / scale
    err = float((got.double().cpu() - ref64).abs().max())
    print(f"{what}: device error {err / scale:.3e} of scale, F {Fl:.3e}, bound {R.bound(Fl):.3e}")
    assert err <= R.bound(Fl, scale), (what, err / scale, Fl)


def _reflect(x, pad):      # [1][C][n]
    return F.pad(x, (pad, pad), mode="reflect")


# -------------------------------------------------------------------------------------------------------- a3t_mgan_stack
@functools.lru_cache(maxsize=None)
def _stack_case(C, dil):
    """Inputs and the CPU references of one ResidualStack, computed once: per row at full length, and rows cut to 257 and (where
    legal) 28 samples run alone, in fp64 and fp32."""
    g = torch.Generator().manual_seed(100 * C + dil)
    x = torch.randn(B, T, C, generator=g)
    w1 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    w2, ws = (torch.randn(C, C, 1, generator=g) / C ** 0.5 for _ in range(2))
    b1, b2, bs = (torch.randn(C, generator=g) * 0.3 for _ in range(3))

    def run(xr, dt):       # xr [n][C] -> [n][C]
        a = xr.to(dt).t()[None]
        h = F.conv1d(_reflect(F.leaky_relu(a, SLOPE), dil), w1.to(dt), b1.to(dt), dilation=dil)
        y = F.conv1d(F.leaky_relu(h, SLOPE), w2.to(dt), b2.to(dt)) + F.conv1d(a, ws.to(dt), bs.to(dt))
        return y[0].t()

    ref = {}
    for dt in (torch.float64, torch.float32):
        ref[dt] = {n: run(x[1, :n], dt) for n in (257, 28) if n > dil}
        ref[dt][T] = torch.stack([run(x[b], dt) for b in range(B)])
    return x, (w1, b1, w2, b2, ws, bs), ref


@pytest.mark.parametrize("dil", [1, 3, 9, 27])
@pytest.mark.parametrize("C", [48, 96, 192])
def test_mgan_stack(C, dil):
    """Dense; ragged with a row end one sample into a tile (257); for dil 27 also the shortest legal row (28), both reflections
    inside one tile.  Nothing behind W_b is written, the input is bit-unchanged, a ragged row is the row run alone bit for bit."""
    from a3t_amd import ops
    from a3t_amd.vocoder import pack_melgan_stack
    x, raw, ref = _stack_case(C, dil)
    w, bias = (t.to(DEV) for t in pack_melgan_stack(*raw))
    xd = x.to(DEV).view(B * T, C)
    keep = xd.clone()
    scale = float(ref[torch.float64][T].abs().max())
    y = torch.full((B * T, C), SENTINEL, device=DEV)
    ops.mgan_stack(xd, w, bias, y, B, T, dil, SLOPE)
    _check(f"mgan_stack C{C} dil{dil} dense", y.view(B, T, C), ref[torch.float64][T], ref[torch.float32][T], scale)
    dense = y.view(B, T, C).clone()
    for W1 in (257, 28) if dil == 27 else (257,):
        tag = f"mgan_stack C{C} dil{dil} ragged ({T}, {W1})"
        y = torch.full((B * T, C), SENTINEL, device=DEV)
        ops.mgan_stack(xd, w, bias, y, B, T, dil, SLOPE, tiles=_tiles([T, W1]), wmin=W1)
        y = y.view(B, T, C)
        assert torch.equal(y[0], dense[0]), tag                                  # the full row: the dense run's bits
        _check(tag, y[1, :W1], ref[torch.float64][W1], ref[torch.float32][W1], scale)
        assert bool((y[1, W1:] == SENTINEL).all()), tag                           # nothing behind W_b is written
        alone = torch.full((W1, C), SENTINEL, device=DEV)
        ops.mgan_stack(x[1, :W1].contiguous().to(DEV), w, bias, alone, 1, W1, dil, SLOPE)
        assert torch.equal(y[1, :W1], alone), (tag, float((y[1, :W1] - alone).abs().max()))
    assert torch.equal(xd, keep)      # the input is bit-unchanged


def test_mgan_stack_refuses_what_it_was_not_built_for():
    from a3t_amd import ops
    from a3t_amd._lib import A3TLibraryError
    from a3t_amd.vocoder import pack_melgan_stack
    C = 48
    x, y = torch.zeros(512, C, device=DEV), torch.zeros(512, C, device=DEV)
    w, bias = (t.to(DEV) for t in pack_melgan_stack(torch.zeros(C, C, 3), None, torch.zeros(C, C, 1), None, torch.zeros(C, C, 1), None))
    with pytest.raises(ValueError, match="overlaps"):
        ops.mgan_stack(x, w, bias, x, 1, 512, 1, SLOPE)                                          # in place on the input
    with pytest.raises(ValueError, match="must be"):
        ops.mgan_stack(x, w[:-1], bias, y, 1, 512, 1, SLOPE)                                     # a row of the operand missing
    with pytest.raises(A3TLibraryError):
        ops.mgan_stack(x, w, bias, y, 1, 512, 0, SLOPE)                                          # dil 0
    with pytest.raises(A3TLibraryError):
        ops.mgan_stack(x, w, bias, y, 1, 512, 512, SLOPE)                                        # dil >= Tw, dense
    with pytest.raises(A3TLibraryError):
        ops.mgan_stack(x, w, bias, y, 2, 256, 27, SLOPE, tiles=_tiles([256, 27]), wmin=27)       # dil >= W_b of a listed row
    with pytest.raises(A3TLibraryError):
        ops.mgan_stack(x, w, bias, y, 2, 256, 27, SLOPE, tiles=_tiles([256, 27]))                # (the same, W_b read from the list)
    x64, y64 = torch.zeros(512, 64, device=DEV), torch.zeros(512, 64, device=DEV)
    with pytest.raises(A3TLibraryError):                                                         # 64 channels
        ops.mgan_stack(x64, torch.zeros(4 * 64 + 64, 64, device=DEV), torch.zeros(2, 64, device=DEV), y64, 1, 512, 1, SLOPE)
    with pytest.raises(ValueError):
        ops.mgan_stack(x, w, bias, y, 1, 512, 1, SLOPE, tiles=torch.zeros(3, 4, dtype=torch.int32, device=DEV))      # 3 tiles in 512 samples
    pad = torch.zeros(9, 4, dtype=torch.int32, device=DEV).view(-1)[4 + 1:4 + 1 + 8].view(2, 4)      # a list 4 bytes off 16
    with pytest.raises(A3TLibraryError):
        ops.mgan_stack(x, w, bias, y, 1, 512, 1, SLOPE, tiles=pad, wmin=512)
    assert bool((y == 0).all())      # nothing was launched


# ---------------------------------------------------------------------------------------------------------- a3t_mgan_out
@pytest.mark.parametrize("tanh", [True, False])
@pytest.mark.parametrize("C,O,K", [(48, 4, 7), (16, 1, 5), (24, 4, 7)])
def test_mgan_out(C, O, K, tanh):
    from a3t_amd import ops
    g = torch.Generator().manual_seed(C + O + K)
    x = torch.randn(B, T, C, generator=g)
    w = torch.randn(O, C, K, generator=g) / (C * K) ** 0.5
    bias = torch.randn(O, generator=g) * 0.1
    W1 = 257

    def run(xr, dt):
        v = F.conv1d(_reflect(F.leaky_relu(xr.to(dt).t()[None], SLOPE), (K - 1) // 2), w.to(dt), bias.to(dt))
        return (torch.tanh(v) if tanh else v)[0].t()

    xd = x.to(DEV).view(B * T, C)
    keep = xd.clone()
    wk, bd = w.permute(0, 2, 1).contiguous().to(DEV), bias.to(DEV)                # [O][K][C]
    for ragged in (False, True):
        ref = []
        for dt in (torch.float64, torch.float32):
            v = torch.stack([run(x[b], dt) for b in range(B)])
            if ragged:
                v[1, :W1] = run(x[1, :W1], dt)
                v[1, W1:] = SENTINEL
            ref.append(v)
        y = torch.full((B * T, O), SENTINEL, device=DEV)
        ops.mgan_out(xd, wk, bd, y, B, T, SLOPE, tanh, tiles=_tiles([T, W1]) if ragged else None, wmin=W1 if ragged else None)
        scale = float(ref[0][0].abs().max())
        _check(f"mgan_out C{C} O{O} K{K} tanh={tanh} {'ragged' if ragged else 'dense'}", y.view(B, T, O), ref[0], ref[1], scale)
        if ragged:
            assert bool((y.view(B, T, O)[1, W1:] == SENTINEL).all())
    assert torch.equal(xd, keep)


# ---------------------------------------------------------------------------------------------------- a3t_pqmf_synthesis
@pytest.mark.parametrize("taps", [62, 30])
def test_pqmf_synthesis(taps):
    """S = 4; Ts 1, 7, 75, 300 dense and a ragged (300, 65) batch, against conv_transpose1d + conv1d in fp64 with the fp32 filter."""
    from a3t_amd import ops
    from a3t_amd.vocoder import pqmf_synthesis_filter
    S = 4
    h = pqmf_synthesis_filter(S, taps, 0.142 if taps == 62 else 0.15, 9.0 if taps == 62 else 8.0)
    hd = torch.from_numpy(h).to(DEV)
    g = torch.Generator().manual_seed(taps)
    for Ts in (1, 7, 75, 300):
        x = torch.randn(B, Ts, S, generator=g)
        ref = [R.pqmf_synthesis(x.to(dt).transpose(1, 2), h).transpose(1, 2) for dt in (torch.float64, torch.float32)]
        y = torch.full((B * Ts * S,), SENTINEL, device=DEV)
        ops.pqmf_synthesis(x.to(DEV).view(B * Ts, S), hd, y, B, Ts)
        _check(f"pqmf taps {taps} Ts {Ts} dense", y.view(B, Ts * S, 1), ref[0], ref[1])
    Ts, W1 = 300, 65
    x = torch.randn(B, Ts, S, generator=g)
    xn = x.clone()
    xn[1, W1:] = float("nan")
    ref = []
    for dt in (torch.float64, torch.float32):
        v = R.pqmf_synthesis(x.to(dt).transpose(1, 2), h).transpose(1, 2).clone()
        v[1, :W1 * S] = R.pqmf_synthesis(x[1:, :W1].to(dt).transpose(1, 2), h).transpose(1, 2)[0]
        v[1, W1 * S:] = SENTINEL
        ref.append(v)
    y = torch.full((B * Ts * S,), SENTINEL, device=DEV)
    ops.pqmf_synthesis(xn.to(DEV).view(B * Ts, S), hd, y, B, Ts, tiles=_tiles([Ts, W1], S))
    _check(f"pqmf taps {taps} ragged", y.view(B, Ts * S, 1), ref[0], ref[1], float(ref[0][0].abs().max()))
    assert bool((y.view(B, Ts * S)[1, W1 * S:] == SENTINEL).all())
    alone = torch.empty(W1 * S, device=DEV)
    ops.pqmf_synthesis(x[1, :W1].contiguous().to(DEV), hd, alone, 1, W1)
    assert torch.equal(y.view(B, Ts * S)[1, :W1 * S], alone)


# -------------------------------------------------------------------------------------------------- a3t_reflect_pad_rows
def test_reflect_pad_rows():
    """Bit-exact against torch; ragged rows (at a rate of 3 samples per frame) reflect at their own ends, an empty row is zeros."""
    from a3t_amd import ops
    from a3t_amd._lib import A3TLibraryError
    C, Tn, pad = 5, 12, 4
    x = torch.randn(3, Tn, C, generator=torch.Generator().manual_seed(1))
    want = F.pad(x.transpose(1, 2), (pad, pad), mode="reflect").transpose(1, 2)
    y = torch.full((3, Tn + 2 * pad, C), SENTINEL, device=DEV)
    ops.reflect_pad_rows(x.to(DEV), y, pad)
    assert torch.equal(y.cpu(), want)
    lens, mul = (4, 2, 0), 3      # rows of 12, 6 and 0 samples
    xn = x.clone()
    xn[1, 6:], xn[2] = float("nan"), float("nan")
    y = torch.full((3, Tn + 2 * pad, C), SENTINEL, device=DEV)
    ops.reflect_pad_rows(xn.to(DEV), y, pad, torch.tensor(lens, dtype=torch.int32, device=DEV), mul)
    y = y.cpu()
    assert torch.equal(y[0], want[0]) and bool((y[2] == 0).all())
    assert torch.equal(y[1, :6 + 2 * pad], F.pad(x[1:2, :6].transpose(1, 2), (pad, pad), mode="reflect").transpose(1, 2)[0])
    assert bool(torch.isfinite(y).all())      # behind a short row's reflected end: clamped into the row
    with pytest.raises(A3TLibraryError):
        ops.reflect_pad_rows(x.to(DEV), torch.empty(3, 3 * Tn, C, device=DEV), Tn)      # pad >= T


# ------------------------------------------------------------------------------------------------------ whole generator
@functools.lru_cache(maxsize=None)
def _state(name):
    c = R.CASES[name]
    return R.procedural_melgan_state(c["cfg"], c["seed"], c["weight_norm"])


@functools.lru_cache(maxsize=None)
def _gen(name, fused):
    from a3t_amd.vocoder import MelGANGeneratorHIP
    return MelGANGeneratorHIP(_state(name), device=DEV, fused=fused, pqmf=R.CASES[name]["pqmf"], **R.CASES[name]["cfg"])


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(G, "melgan.npz")), json.load(open(os.path.join(G, "melgan.json")))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_generator_against_the_reference(name, fused):
    arrays, meta = _golden()
    gen, case, info = _gen(name, fused), R.CASES[name], meta["cases"][name]
    assert gen.fused == fused and gen.min_frames == info["min_frames"]
    if name == "mb_v2_wn":
        assert all(st["fused"] == fused for st in gen.stages) and gen.fused_out == fused
    for Tf in case["frames"]:
        want = arrays[f"{name}.T{Tf}.wav64"]
        got = gen.inference(torch.from_numpy(R.mel_input(Tf, case["seed"]))).cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        err, bound = float(np.abs(got - want).max()), R.bound(info["F"][str(Tf)], R.scale_of(want))
        print(f"generator {name} fused={fused} T={Tf}: device error {err:.3e}, F {info['F'][str(Tf)]:.3e}, bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("name", list(R.CASES))
def test_ragged_batch_equals_the_single_runs(name):
    """The three fixture lengths and an empty row, NaN in the padding of c: every row is its single run bit for bit in both modes,
    and the fused rows are the layer-by-layer rows within the fixture's bound."""
    case, info = R.CASES[name], _golden()[1]["cases"][name]
    hop, lengths = info["hop"], tuple(case["frames"]) + (0,)
    Tm = max(lengths)
    c = torch.full((4, Tm, 80), float("nan"))
    for b, n in enumerate(lengths):
        c[b, :n] = torch.from_numpy(R.mel_input(n, case["seed"]))
    out = {}
    for fused in (False, True):
        gen = _gen(name, fused)
        keep = c.clone().to(DEV)
        cd = keep.clone()
        y = gen.inference(cd, lengths=lengths)
        assert y.shape == (4, Tm * hop, 1) and torch.equal(torch.isnan(cd), torch.isnan(keep))      # the caller's tensor is untouched
        for b, n in enumerate(lengths):
            if n:
                alone = gen.inference(c[b, :n])
                assert torch.equal(y[b, :n * hop], alone), (fused, b, float((y[b, :n * hop] - alone).abs().max()))
            assert bool((y[b, n * hop:] == 0).all())
        out[fused] = y.cpu().double()
    for b, n in enumerate(lengths[:3]):
        err = float((out[True][b] - out[False][b]).abs().max())
        bound = R.bound(info["F"][str(n)], R.scale_of(out[False][b].numpy()))
        print(f"ragged {name} row {b} ({n} frames): fused vs layer by layer {err:.3e}, bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("fused", [False, True])
def test_span_window_reproduces_the_full_run(fused):
    """A window of margin_frames reproduces the span bit for bit: mid-utterance, and at both ends, where the window is clipped
    and its reflection is the utterance's own."""
    from a3t_amd.vocoder import span_window
    gen, hop = _gen("mb_v2_wn", fused), 300
    m, Tn = gen.margin_frames, 48
    assert m == 15 and gen.upsample_factor == hop
    c = torch.from_numpy(R.mel_input(Tn, 9)).to(DEV)
    full = gen.inference(c)
    wins = []
    for n0, n1 in ((20, 23), (0, 3), (45, 48)):
        w0, w1 = span_window(n0, n1, Tn, m)
        assert (w0, w1) == R.window(n0, n1, Tn, m)
        win = gen.inference(c[w0:w1])
        assert torch.equal(win[(n0 - w0) * hop:(n1 - w0) * hop], full[n0 * hop:n1 * hop]), (n0, n1)
        wins.append((n0, n1, w0, w1))
    # the same spans as the rows of one ragged batch of windows
    rows = torch.zeros(3, max(w1 - w0 for *_, w0, w1 in wins), 80, device=DEV)
    for b, (_, _, w0, w1) in enumerate(wins):
        rows[b, :w1 - w0] = c[w0:w1]
    rag = gen.inference(rows, lengths=[w1 - w0 for *_, w0, w1 in wins])
    for b, (n0, n1, w0, w1) in enumerate(wins):
        assert torch.equal(rag[b, (n0 - w0) * hop:(n1 - w0) * hop], full[n0 * hop:n1 * hop])


def test_a_row_of_less_than_min_frames_is_refused_before_any_launch():
    gen = _gen("mb_v2_wn", True)
    assert gen.min_frames == 6
    with pytest.raises(ValueError, match="min_frames"):
        gen.inference(torch.zeros(5, 80))
    with pytest.raises(ValueError, match="min_frames"):
        gen.inference(torch.zeros(2, 9, 80), lengths=(9, 5))
    y = gen.inference(torch.zeros(2, 9, 80), lengths=(9, 0))      # an empty row is legal
    assert bool((y[1] == 0).all()) and bool(torch.isfinite(y).all())


# --------------------------------------------------------------------------------------------------------- SpeechEditor
@functools.lru_cache(maxsize=None)
def _editor():
    import test_gpu_sedit_batch as SB
    ed, oc, *_ = SB._editor()      # a fresh editor of our own (that helper is not cached): replacing its vocoder touches no other test
    assert oc.hop_length == 300
    ed.vocoder = _gen("mb_v2_wn", True)
    return ed, SB


def test_speech_editor_batch_of_one_equals_edit():
    ed, SB = _editor()
    for r in SB._requests():
        one = ed.edit(*SB._args(r), **SB._opts(r))
        got = ed.edit_batch([r])[0]
        assert got["new_span_boundary"] == one["new_span_boundary"] and torch.equal(got["feat"], one["feat"])
        for k in ("origin", "prediction", "orgin_replaced"):
            assert np.array_equal(got[k], one[k]), (k, float(np.abs(got[k] - one[k]).max()))
        assert np.isfinite(got["prediction"]).all() and float(np.abs(got["prediction"]).max()) > 1e-3


def test_speech_editor_span_only_equals_full_vocoding():
    ed, SB = _editor()
    reqs = SB._requests()
    full = ed.edit_batch(reqs)
    span = ed.edit_batch(reqs, outputs=("orgin_replaced",))
    assert len(full) == len(span) == 4
    for f, s in zip(full, span):
        assert "prediction" not in s and "prediction" in f
        assert np.array_equal(f["orgin_replaced"], s["orgin_replaced"])
