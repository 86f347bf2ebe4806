"""HiFi-GAN generator on the device (a3t_amd/vocoder.py::HiFiGANGeneratorHIP, csrc/hifigan.hip): the three kernels against fp64
torch, the transposed convolution through the packed GEMM path, the whole generator layer by layer and fused against the
reference's outputs (tests/golden/hifigan.{npz,json}), ragged batches, span windows and SpeechEditor with this vocoder.

Tolerance of every numeric comparison: the yardstick is the fp64 result, the bound 4 x F (hifigan_ref.bound), where F is what an
fp32 evaluation by the reference (fixture cases) or by torch on the CPU (kernel cases, computed here) loses against fp64 on the
same input, floored at 1e-6 of scale: both sides are fp32 evaluations of the same sums in different orders, and the comparison
takes the worst of several thousand samples.  Measured device values: profiles/hifigan_parity.txt."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hifigan_ref as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
B, T, W = 2, 700, (700, 259)      # partial tiles (700 = 2 * 256 + 188) and a row end inside a tile (259 = 256 + 3)
SENTINEL = 7.5


def _tiles(lengths, rate=1):
    from a3t_amd.vocoder import pwg_tile_list
    return torch.from_numpy(pwg_tile_list(lengths, rate)).to(DEV)


def _leaky(x, slope):
    return torch.where(x > 0, x, x * slope)


def _check(what, got, ref64, ref32, scale=None):
    """got (device fp32) against ref64 within 4 x F, F from ref32 (the CPU's fp32 evaluation)."""
    scale = float(ref64.abs().max()) if scale is None else scale
    Fl = float((ref32.double() - ref64).abs().max()) / scale
    err = float((got.double().cpu() - ref64).abs().max())
    print(f"{what}: device error {err / scale:.3e} of scale, F {Fl:.3e}, bound {R.bound(Fl):.3e}")
    assert err <= R.bound(Fl, scale), (what, err / scale, Fl)


# --------------------------------------------------------------------------------------------------------- a3t_hfg_conv
@functools.lru_cache(maxsize=None)
def _conv_case(C, k, dil):
    """Inputs and the CPU references of one convolution, computed once: v = bias + conv(leaky(x)) per row, dense and with row
    1 cut to W[1] samples (run alone), in fp64 and fp32."""
    g = torch.Generator().manual_seed(1000 * C + 10 * k + dil)
    x = torch.randn(B, T, C, generator=g)
    w = torch.randn(C, C, k, generator=g) / (C * k) ** 0.5
    bias = torch.randn(C, generator=g)
    res = torch.randn(B, T, C, generator=g)
    acc0 = torch.randn(B, T, C, generator=g)

    def conv(xr, dt):       # xr [n][C] -> [n][C]
        a = _leaky(xr.to(dt), 0.1).t()[None]
        return F.conv1d(a, w.to(dt), bias.to(dt), padding=(k - 1) // 2 * dil, dilation=dil)[0].t()

    ref = {}
    for dt in (torch.float64, torch.float32):
        dense = torch.stack([conv(x[b], dt) for b in range(B)])
        ragged = dense.clone()
        ragged[1, :W[1]] = conv(x[1, :W[1]], dt)
        ref[dt] = (dense, ragged)
    return x, w, bias, res, acc0, ref


CONV_CASES = [(C, k, d) for C in (32, 64) for k in (3, 7, 11) for d in (1, 5)] + [(64, 11, 27), (32, 3, 300)]


@pytest.mark.parametrize("C,k,dil", CONV_CASES)
def test_hfg_conv(C, k, dil):
    """(dil 27, k 11: a halo of 135 samples, more than half a tile; dil 300, k 3: taps a whole tile and more away.)"""
    from a3t_amd import ops
    from a3t_amd.vocoder import pack_hifigan_conv
    x, w, bias, res, acc0, ref = _conv_case(C, k, dil)
    xd, rd = x.to(DEV).view(B * T, C), res.to(DEV).view(B * T, C)
    wt, bd = pack_hifigan_conv(w).to(DEV), bias.to(DEV)
    keep = xd.clone()
    for ragged in (False, True):
        tiles = _tiles([W[0], W[1]]) if ragged else None
        v64, v32 = (ref[dt][int(ragged)] for dt in (torch.float64, torch.float32))
        valid = torch.zeros(B, T, 1, dtype=torch.bool)
        for b in range(B):
            valid[b, :(W[b] if ragged else T)] = True
        tag = f"C{C} k{k} dil{dil} {'ragged' if ragged else 'dense'}"
        scale = float(v64.abs().max())

        def expect(v, fill):
            return torch.where(valid, v, torch.as_tensor(fill, dtype=v.dtype))

        # store, no residual
        y = torch.full((B * T, C), SENTINEL, device=DEV)
        ops.hfg_conv(xd, wt, bd, y, B, T, dil, 0.1, tiles=tiles)
        _check(tag + " store", y.view(B, T, C), expect(v64, SENTINEL), expect(v32, SENTINEL), scale)
        assert bool((y.view(B, T, C).cpu()[~valid.expand(B, T, C)] == SENTINEL).all())
        # store with a separate residual (what every unit but a block's last does: y = xn, R = x)
        y = torch.full((B * T, C), SENTINEL, device=DEV)
        ops.hfg_conv(xd, wt, bd, y, B, T, dil, 0.1, R=rd, tiles=tiles)
        want = [expect(v.to(dt) + res.to(dt), SENTINEL) for v, dt in ((v64, torch.float64), (v32, torch.float32))]
        _check(tag + " store with residual", y.view(B, T, C), want[0], want[1], scale)
        assert torch.equal(rd, res.to(DEV).view(B * T, C))
        # accumulate only, no residual
        acc = acc0.to(DEV).view(B * T, C).clone()
        ops.hfg_conv(xd, wt, bd, None, B, T, dil, 0.1, acc=acc, alpha=0.5, acc_add=True, tiles=tiles)
        want = [torch.where(valid, acc0.to(dt) + 0.5 * v.to(dt), acc0.to(dt)) for v, dt in ((v64, torch.float64), (v32, torch.float32))]
        _check(tag + " accumulate", acc.view(B, T, C), want[0], want[1], scale)
        # residual, accumulate only (acc = alpha * v, then acc += alpha * v)
        acc = acc0.to(DEV).view(B * T, C).clone()
        ops.hfg_conv(xd, wt, bd, None, B, T, dil, 0.1, R=rd, acc=acc, alpha=0.25, tiles=tiles)
        ops.hfg_conv(xd, wt, bd, None, B, T, dil, 0.1, R=rd, acc=acc, alpha=0.5, acc_add=True, tiles=tiles)
        want = [torch.where(valid, 0.75 * (v.to(dt) + res.to(dt)), acc0.to(dt)) for v, dt in ((v64, torch.float64), (v32, torch.float32))]
        _check(tag + " residual accumulate", acc.view(B, T, C), want[0], want[1], scale)
        assert torch.equal(acc.view(B, T, C).cpu()[~valid.expand(B, T, C)], acc0[~valid.expand(B, T, C)])
        # both, in place on the residual (y aliases R)
        y = rd.clone()
        acc = acc0.to(DEV).view(B * T, C).clone()
        ops.hfg_conv(xd, wt, bd, y, B, T, dil, 0.1, R=y, acc=acc, alpha=1.0, acc_add=True, tiles=tiles)
        want = [torch.where(valid, v.to(dt) + res.to(dt), res.to(dt)) for v, dt in ((v64, torch.float64), (v32, torch.float32))]
        _check(tag + " both: y", y.view(B, T, C), want[0], want[1], scale)
        want = [torch.where(valid, acc0.to(dt) + v.to(dt) + res.to(dt), acc0.to(dt)) for v, dt in ((v64, torch.float64), (v32, torch.float32))]
        _check(tag + " both: acc", acc.view(B, T, C), want[0], want[1], scale)
        # no bias
        y = torch.full((B * T, C), SENTINEL, device=DEV)
        ops.hfg_conv(xd, wt, None, y, B, T, dil, 0.1, tiles=tiles)
        _check(tag + " no bias", y.view(B, T, C), expect(v64 - bias.double(), SENTINEL), expect(v32 - bias, SENTINEL), scale)
    assert torch.equal(xd, keep)      # the input is bit-unchanged


def test_hfg_conv_refuses_what_it_was_not_built_for():
    from a3t_amd import ops
    from a3t_amd._lib import A3TLibraryError
    x, y = torch.zeros(512, 32, device=DEV), torch.zeros(512, 32, device=DEV)
    w = torch.zeros(3 * 32, 32, device=DEV)
    with pytest.raises(ValueError, match="overlaps"):
        ops.hfg_conv(x, w, None, x, 1, 512, 1, 0.1)                       # in place on the input
    with pytest.raises(ValueError, match="overlaps"):
        ops.hfg_conv(x, w, None, y, 1, 512, 1, 0.1, acc=y)                # y and acc the same buffer
    with pytest.raises(ValueError, match="must be"):
        ops.hfg_conv(x, w, None, y.view(256, 64), 1, 512, 1, 0.1)         # the right size, another trailing dimension
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv(x, w, None, y, 1, 512, 0, 0.1)                       # dil 0
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv(x, torch.zeros(4 * 32, 32, device=DEV), None, y, 1, 512, 1, 0.1)      # even kernel
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv(x, torch.zeros(13 * 32, 32, device=DEV), None, y, 1, 512, 1, 0.1)     # kernel > 11
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv(torch.zeros(512, 48, device=DEV), torch.zeros(3 * 48, 48, device=DEV), None, torch.zeros(512, 48, device=DEV),
                     1, 512, 1, 0.1)                                       # 48 channels
    with pytest.raises(ValueError):
        ops.hfg_conv(x, w, None, y, 1, 512, 1, 0.1, tiles=torch.zeros(3, 4, dtype=torch.int32, device=DEV))   # 3 tiles in 512 samples


# ---------------------------------------------------------------------------------------------- a3t_hfg_out, a3t_leaky_relu
@pytest.mark.parametrize("C,K,slope", [(32, 7, 0.01), (64, 7, 0.1), (32, 11, 0.1), (4, 7, 0.01), (64, 11, 0.01)])
def test_hfg_out(C, K, slope):
    from a3t_amd import ops
    g = torch.Generator().manual_seed(C + K)
    x = torch.randn(B, T, C, generator=g)
    w = torch.randn(1, C, K, generator=g) / (C * K) ** 0.5
    bias = torch.randn(1, generator=g) * 0.1

    def run(xr, dt):
        return torch.tanh(F.conv1d(_leaky(xr.to(dt), slope).t()[None], w.to(dt), bias.to(dt), padding=(K - 1) // 2))[0].t()

    xd = x.to(DEV).view(B * T, C)
    keep = xd.clone()
    wk, bd = w[0].t().contiguous().to(DEV), bias.to(DEV)                # [K][C]
    for ragged in (False, True):
        ref = []
        for dt in (torch.float64, torch.float32):
            v = torch.stack([run(x[b], dt) for b in range(B)])
            if ragged:
                v[1, :W[1]] = run(x[1, :W[1]], dt)
                v[1, W[1]:] = SENTINEL
            ref.append(v)
        y = torch.full((B * T,), SENTINEL, device=DEV)
        ops.hfg_out(xd, wk, bd, y, B, T, slope, tiles=_tiles(W) if ragged else None)
        _check(f"hfg_out C{C} K{K} slope {slope} {'ragged' if ragged else 'dense'}", y.view(B, T, 1), ref[0], ref[1], 1.0)
        if ragged:
            assert bool((y.view(B, T)[1, W[1]:] == SENTINEL).all())
    assert torch.equal(xd, keep)


def test_hfg_out_row_shorter_than_its_halo():
    """A row of 2 samples under K = 7 (halo 3): every tap beyond the row is ZERO padding.  The kernel is shared with
    a3t_mgan_out, whose taps reflect at the row's ends; on this row the two paddings differ at every sample."""
    from a3t_amd import ops
    C, K, slope, Bs, Ts, Ws = 32, 7, 0.1, 2, 300, (300, 2)
    g = torch.Generator().manual_seed(C + K + Ts)
    x = torch.randn(Bs, Ts, C, generator=g)
    w = torch.randn(1, C, K, generator=g) / (C * K) ** 0.5
    bias = torch.randn(1, generator=g) * 0.1

    def run(xr, dt):
        return torch.tanh(F.conv1d(_leaky(xr.to(dt), slope).t()[None], w.to(dt), bias.to(dt), padding=(K - 1) // 2))[0].t()

    xd = x.to(DEV).view(Bs * Ts, C)
    wk, bd = w[0].t().contiguous().to(DEV), bias.to(DEV)                # [K][C]
    for ragged in (False, True):
        ref = []
        for dt in (torch.float64, torch.float32):
            v = torch.stack([run(x[b], dt) for b in range(Bs)])
            if ragged:
                v[1, :Ws[1]] = run(x[1, :Ws[1]], dt)
                v[1, Ws[1]:] = SENTINEL
            ref.append(v)
        y = torch.full((Bs * Ts,), SENTINEL, device=DEV)
        ops.hfg_out(xd, wk, bd, y, Bs, Ts, slope, tiles=_tiles(Ws) if ragged else None)
        _check(f"hfg_out short row {'ragged' if ragged else 'dense'}", y.view(Bs, Ts, 1), ref[0], ref[1], 1.0)
        if ragged:
            assert bool((y.view(Bs, Ts)[1, Ws[1]:] == SENTINEL).all())


@pytest.mark.parametrize("slope", [0.1, 0.01])
def test_leaky_relu(slope):
    """Exact: one fp32 multiplication.  A length that is no multiple of 4 (the 16-byte body and its tail), an unaligned view
    (the scalar path), in place."""
    from a3t_amd import ops
    x = torch.randn(B * T * 32 + 3, generator=torch.Generator().manual_seed(3))
    x[:4] = torch.tensor([0.0, -0.0, 1.0, -1.0])
    want = F.leaky_relu(x, slope)
    xd = x.to(DEV)
    y = torch.full_like(xd, SENTINEL)
    ops.leaky_relu(xd, y, slope)
    assert torch.equal(y.cpu(), want) and torch.equal(xd.cpu(), x)
    buf = torch.full((x.numel() + 2,), SENTINEL, device=DEV)
    ops.leaky_relu(xd[1:], buf[2:-1], slope)      # 4 and 8 bytes off a 16-byte boundary
    assert torch.equal(buf[2:-1].cpu(), want[1:]) and float(buf[0]) == SENTINEL and float(buf[1]) == SENTINEL and float(buf[-1]) == SENTINEL
    ops.leaky_relu(xd, xd, slope)
    assert torch.equal(xd.cpu(), want)


# ------------------------------------------------------------------------------- transposed convolution on the packed GEMM
@pytest.mark.parametrize("s", [5, 4, 3])
def test_transposed_convolution_through_the_packed_gemm(s):
    from a3t_amd import ops
    from a3t_amd._lib import F32
    from a3t_amd.vocoder import pack_hifigan_upsample
    g = torch.Generator().manual_seed(s)
    Cin, Cout, Tf = 64, 32, 37
    x = torch.randn(B, Tf, Cin, generator=g)
    w = torch.randn(Cin, Cout, 2 * s, generator=g) / (2 * Cin) ** 0.5
    bias = torch.randn(Cout, generator=g)
    ref = [F.conv_transpose1d(x.to(dt).transpose(1, 2), w.to(dt), bias.to(dt), stride=s, padding=s // 2 + s % 2,
                              output_padding=s % 2).transpose(1, 2) for dt in (torch.float64, torch.float32)]
    out = torch.empty(B * Tf, s * Cout, device=DEV)
    ops.conv_fwd(x.to(DEV).view(B * Tf, Cin), pack_hifigan_upsample(w, s).to(DEV), out, Tf, 1, bias=bias.repeat(s).to(DEV), compute=F32)
    _check(f"transposed convolution s={s}", out.view(B, Tf * s, Cout), ref[0], ref[1])


# ------------------------------------------------------------------------------------------------------ whole generator
@functools.lru_cache(maxsize=None)
def _state(name):
    c = R.CASES[name]
    return R.procedural_hifigan_state(c["cfg"], c["seed"], c["weight_norm"])


@functools.lru_cache(maxsize=None)
def _gen(name, fused):
    from a3t_amd.vocoder import HiFiGANGeneratorHIP
    return HiFiGANGeneratorHIP(_state(name), device=DEV, fused=fused, **R.CASES[name]["cfg"])


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_generator_against_the_reference(name, fused):
    arrays, meta = np.load(os.path.join(G, "hifigan.npz")), json.load(open(os.path.join(G, "hifigan.json")))
    gen, case, info = _gen(name, fused), R.CASES[name], meta["cases"][name]
    assert gen.fused == fused      # every fixture plan has a stage of 32 or 64 channels
    for Tf in R.FRAMES:
        want = arrays[f"{name}.T{Tf}.wav64"]
        got = gen.inference(torch.from_numpy(R.mel_input(Tf, case["seed"]))).cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        err, bound = float(np.abs(got - want).max()), R.bound(info["F"][str(Tf)], R.scale_of(want))
        print(f"generator {name} fused={fused} T={Tf}: device error {err:.3e}, F {info['F'][str(Tf)]:.3e}, bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["v1_wn", "odd"])
def test_ragged_batch_equals_the_single_runs(name, fused):
    gen, hop = _gen(name, fused), R.hop_of(R.CASES[name]["cfg"])
    lengths = (13, 1, 7)
    c = torch.full((3, 13, 80), float("nan"))
    for b, n in enumerate(lengths):
        c[b, :n] = torch.from_numpy(R.mel_input(n, 50 + b))
    keep = c.clone().to(DEV)
    cd = keep.clone()
    y = gen.inference(cd, lengths=lengths)
    assert y.shape == (3, 13 * hop, 1) and torch.equal(torch.isnan(cd), torch.isnan(keep))      # the caller's tensor is untouched
    for b, n in enumerate(lengths):
        alone = gen.inference(c[b, :n])
        assert torch.equal(y[b, :n * hop], alone), (b, float((y[b, :n * hop] - alone).abs().max()))
        assert bool((y[b, n * hop:] == 0).all())
    with pytest.raises(ValueError, match="lengths"):
        gen.inference(cd, lengths=(13, 14, 7))


@pytest.mark.parametrize("fused", [False, True])
def test_span_window_reproduces_the_full_run(fused):
    from a3t_amd.vocoder import span_window
    gen, hop = _gen("v1_wn", fused), 300
    m = gen.margin_frames
    assert m in (19, 20) and gen.upsample_factor == hop
    c = torch.from_numpy(R.mel_input(60, 9)).to(DEV)
    full = gen.inference(c)
    n0, n1 = 25, 28
    w0, w1 = span_window(n0, n1, 60, m)
    assert (w0, w1) == R.window(n0, n1, 60, m) == (n0 - m, n1 + m)
    win = gen.inference(c[w0:w1])
    assert torch.equal(win[(n0 - w0) * hop:(n1 - w0) * hop], full[n0 * hop:n1 * hop])
    # the same span as a row of a ragged batch of windows
    rows = torch.zeros(2, w1 - w0, 80, device=DEV)
    rows[0], rows[1, :5] = c[w0:w1], c[:5]
    rag = gen.inference(rows, lengths=(w1 - w0, 5))
    assert torch.equal(rag[0, (n0 - w0) * hop:(n1 - w0) * hop], full[n0 * hop:n1 * hop])


# --------------------------------------------------------------------------------------------------------- SpeechEditor
@functools.lru_cache(maxsize=None)
def _editor():
    import test_gpu_sedit_batch as SB
    ed, oc, *_ = SB._editor()      # a fresh editor of our own (that helper is not cached): replacing its vocoder touches no PWG test
    assert oc.hop_length == 300
    ed.vocoder = _gen("v1_wn", True)
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
