"""HiFiGANGeneratorHIP(compute="f16") on the device (a3t_amd/csrc/hifigan_f16.hip): a3t_hfg_conv_f16 against the restatement of
one convolution with fp16 rounding (tests/hifigan_f16_ref.py), the whole generator against the reference's fp64 outputs
(tests/golden/hifigan.npz) within what the CPU restatement with fp16 operands loses, ragged rows and span windows bit for bit,
determinism, the untouched default, a hot input, the entry point's refusals and SpeechEditor with this vocoder."""
import functools
import os

import numpy as np
import pytest
import torch

import hifigan_ref as R
import hifigan_f16_ref as H

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
B, T, W = 2, 600, (600, 257)      # two full tiles and a partial one (600 = 2 * 256 + 88); a tile with one valid sample (257)
SENTINEL = 7.5
SLOPE = 0.1
ALPHA = float(np.float32(1.0 / 3.0))


def _tiles(lengths, rate=1):
    from a3t_amd.vocoder import pwg_tile_list
    return torch.from_numpy(pwg_tile_list(lengths, rate)).to(DEV)


# ----------------------------------------------------------------------------------------------------- a3t_hfg_conv_f16
@functools.lru_cache(maxsize=None)
def _conv_case(C, k, dil):
    """Inputs (x = 1.5 N(0, 1), procedural weights) and the fp64-accumulated restatements of one convolution, with fp16 rounding
    and without: per row, dense and with row 1 cut to W[1] samples (run alone)."""
    from oracle.a3t_oracle import procedural_state
    st = procedural_state({"w": (C, C, k), "b": (C,)}, seed=1000 * C + 10 * k + dil)
    w, bias = torch.from_numpy(st["w"]).float(), torch.from_numpy(st["b"]).float()
    g = torch.Generator().manual_seed(C + k + dil)
    x = 1.5 * torch.randn(B, T, C, generator=g)
    res = torch.randn(B, T, C, generator=g)
    acc0 = torch.randn(B, T, C, generator=g)
    ref = {}
    for rnd in (torch.float16, None):
        dense = torch.stack([H.conv_unit(x[b], w, bias, dil, SLOPE, rnd)[0] for b in range(B)])
        ragged = dense.clone()
        ragged[1, :W[1]] = H.conv_unit(x[1, :W[1]], w, bias, dil, SLOPE, rnd)[0]
        ref[rnd] = (dense, ragged)
    return x, w, bias, res, acc0, ref


@pytest.mark.parametrize("dil", [1, 27, 300])
@pytest.mark.parametrize("k", [3, 11])
@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_hfg_conv_f16(C, k, dil):
    """RMS(kernel - restatement with fp16 rounding, accumulated in fp64) <= 0.1 x RMS(that restatement - the unrounded one), the
    ratio of test_gpu_vocoder_f16.py: what may remain is the fp32 accumulation order, about 1e-3 of the rounding.  (dil 300: the
    taps are more than a tile away; at k = 11 all but the centre tap of most samples are outside the row.)"""
    from a3t_amd import ops
    from a3t_amd.vocoder import pack_hifigan_conv_f16
    x, w, bias, res, acc0, ref = _conv_case(C, k, dil)
    xd = x.to(DEV).view(B * T, C)
    wf, bd = pack_hifigan_conv_f16(w).to(DEV), bias.to(DEV)
    keep = xd.clone()
    res64, acc64 = res.double(), acc0.double()
    for ragged in (False, True):
        tiles = _tiles(W) if ragged else None
        v16, v = ref[torch.float16][int(ragged)], ref[None][int(ragged)]
        valid = torch.zeros(B, T, 1, dtype=torch.bool)
        for b in range(B):
            valid[b, :(W[b] if ragged else T)] = True
        vm = valid.expand(B, T, C)
        tag = f"C{C} k{k} dil{dil} {'ragged' if ragged else 'dense'}"

        def check(what, got, want16, want):
            got = got.view(B, T, C).cpu().double()
            assert bool(torch.isfinite(got).all())
            r, rounding = H.rms((got - want16)[vm].numpy()), H.rms((want16 - want)[vm].numpy())
            print(f"{tag} {what}: RMS(kernel - restatement) {r:.3e}, RMS(restatement - unrounded) {rounding:.3e}, "
                  f"ratio {r / rounding:.5f}")
            assert rounding > 0 and r <= 0.1 * rounding, (tag, what, r, rounding)
            return got

        # y only
        y = torch.full((B * T, C), SENTINEL, device=DEV)
        ops.hfg_conv_f16(xd, wf, bd, y, B, T, dil, SLOPE, tiles=tiles)
        got = check("y", y, v16, v)
        assert bool((got[~vm] == SENTINEL).all())
        # y + R, R aliasing y
        y = res.to(DEV).view(B * T, C).clone()
        ops.hfg_conv_f16(xd, wf, bd, y, B, T, dil, SLOPE, R=y, tiles=tiles)
        got = check("y with R = y", y, v16 + res64, v + res64)
        assert torch.equal(got[~vm], res64[~vm])
        # acc only, alpha = 1/3
        acc = torch.full((B * T, C), SENTINEL, device=DEV)
        ops.hfg_conv_f16(xd, wf, bd, None, B, T, dil, SLOPE, acc=acc, alpha=ALPHA, tiles=tiles)
        got = check("acc = alpha v", acc, ALPHA * v16, ALPHA * v)
        assert bool((got[~vm] == SENTINEL).all())
        # acc_add, with a residual and y beside it
        acc, y = acc0.to(DEV).view(B * T, C).clone(), torch.full((B * T, C), SENTINEL, device=DEV)
        rd = res.to(DEV).view(B * T, C)
        ops.hfg_conv_f16(xd, wf, bd, y, B, T, dil, SLOPE, R=rd, acc=acc, alpha=ALPHA, acc_add=True, tiles=tiles)
        got = check("acc += alpha v", acc, acc64 + ALPHA * (v16 + res64), acc64 + ALPHA * (v + res64))
        assert torch.equal(got[~vm], acc64[~vm])
        check("y beside acc", y, v16 + res64, v + res64)
        assert torch.equal(rd.cpu(), res.view(B * T, C))
    assert torch.equal(xd, keep)      # the input is bit-unchanged


def test_hfg_conv_f16_refuses_what_it_was_not_built_for():
    from a3t_amd import ops
    from a3t_amd._lib import A3TLibraryError
    from a3t_amd.vocoder import pack_hifigan_conv_f16
    n = 512
    x, y = torch.zeros(n, 32, device=DEV), torch.zeros(n, 32, device=DEV)
    wf = pack_hifigan_conv_f16(torch.zeros(32, 32, 3)).to(DEV)

    def frags(C, k):      # a weight operand of the right trailing shape for any C and k
        return torch.zeros(k * C // 16, C // 32, 64, 8, dtype=torch.float16, device=DEV)

    with pytest.raises(ValueError, match="overlaps"):
        ops.hfg_conv_f16(x, wf, None, x, 1, n, 1, SLOPE)                                    # in place on the input
    with pytest.raises(ValueError, match="overlaps"):
        ops.hfg_conv_f16(x, wf, None, None, 1, n, 1, SLOPE, acc=x)                          # acc is the input
    with pytest.raises(ValueError, match="overlaps"):
        ops.hfg_conv_f16(x, wf, None, y, 1, n, 1, SLOPE, acc=y)                             # y and acc the same buffer
    with pytest.raises(ValueError, match="wf must be"):
        ops.hfg_conv_f16(x, wf.float(), None, y, 1, n, 1, SLOPE)                            # fp32 weights
    with pytest.raises(ValueError, match="wf must be"):
        ops.hfg_conv_f16(x, wf.view(-1, 64, 8), None, y, 1, n, 1, SLOPE)                    # not the fragment shape
    with pytest.raises(ValueError, match="wf must be"):
        ops.hfg_conv_f16(torch.zeros(n, 48, device=DEV), wf, None, torch.zeros(n, 48, device=DEV), 1, n, 1, SLOPE)   # 48 channels
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv_f16(torch.zeros(n, 96, device=DEV), frags(96, 3), None, torch.zeros(n, 96, device=DEV), 1, n, 1, SLOPE)
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv_f16(torch.zeros(n, 512, device=DEV), frags(512, 3), None, torch.zeros(n, 512, device=DEV), 1, n, 1, SLOPE)
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv_f16(x, frags(32, 4), None, y, 1, n, 1, SLOPE)                          # even kernel
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv_f16(x, frags(32, 13), None, y, 1, n, 1, SLOPE)                         # kernel > 11
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv_f16(x, wf, None, y, 1, n, 0, SLOPE)                                    # dil 0
    xbuf = torch.zeros(n * 32 + 4, device=DEV)
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv_f16(xbuf[1:1 + n * 32].view(n, 32), wf, None, y, 1, n, 1, SLOPE)       # x 4 bytes off a 16-byte boundary
    wbuf = torch.zeros(wf.numel() + 8, dtype=torch.float16, device=DEV)
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv_f16(x, wbuf[2:2 + wf.numel()].view(wf.shape), None, y, 1, n, 1, SLOPE)  # the weight 4 bytes off
    tl = _tiles([n]).cpu()
    tbuf = torch.zeros(tl.numel() + 1, dtype=torch.int32, device=DEV)
    tbuf[1:] = tl.reshape(-1).to(DEV)
    with pytest.raises(A3TLibraryError):
        ops.hfg_conv_f16(x, wf, None, y, 1, n, 1, SLOPE, tiles=tbuf[1:].view(-1, 4))        # a misaligned tile list
    with pytest.raises(ValueError):
        ops.hfg_conv_f16(x, wf, None, y, 1, n, 1, SLOPE, tiles=torch.zeros(3, 4, dtype=torch.int32, device=DEV))   # 3 tiles in 512 samples
    y.fill_(SENTINEL)
    ops.hfg_conv_f16(x, wf, None, y, 1, n, 1, SLOPE, tiles=_tiles([n]))                     # the good call goes through
    assert bool((y == 0).all())


# ------------------------------------------------------------------------------------------------------ whole generator
@functools.lru_cache(maxsize=None)
def _state(name):
    c = R.CASES[name]
    return R.procedural_hifigan_state(c["cfg"], c["seed"], c["weight_norm"])


@functools.lru_cache(maxsize=None)
def _gen(name, compute="f16"):
    from a3t_amd.vocoder import HiFiGANGeneratorHIP
    kw = {} if compute is None else dict(compute=compute)
    return HiFiGANGeneratorHIP(_state(name), device=DEV, **kw, **R.CASES[name]["cfg"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_generator_f16_against_the_reference(name):
    """Against the reference's fp64 outputs: RMS and worst-element error each <= 2 x what the CPU restatement with fp16 operands
    loses on the same input, and below the bf16 restatement's (the rules of test_gpu_vocoder_f16.py)."""
    arrays = np.load(os.path.join(G, "hifigan.npz"))
    gen, case = _gen(name), R.CASES[name]
    assert gen.compute == "f16" and any(st["f16"] for st in gen.stages)
    for Tf in R.FRAMES:
        want = arrays[f"{name}.T{Tf}.wav64"]
        mel = torch.from_numpy(R.mel_input(Tf, case["seed"]))
        r16, rb = (H.errors(H.generator(_state(name), case["cfg"], mel, dtype=torch.float32, rnd_dtype=dt).numpy(), want)
                   for dt in (torch.float16, torch.bfloat16))
        got = gen.inference(mel)
        assert got.shape == want.shape and bool(torch.isfinite(got).all())
        e = H.errors(got.cpu().numpy(), want)
        print(f"generator {name} compute=f16 T={Tf}: RMS {e[0]:.3e}, worst {e[1]:.3e}; CPU fp16 restatement {r16[0]:.3e}, {r16[1]:.3e}; "
              f"CPU bf16 restatement {rb[0]:.3e}, {rb[1]:.3e}")
        assert e[0] <= 2 * r16[0] and e[1] <= 2 * r16[1]
        assert e[0] < rb[0] and e[1] < rb[1]
        # the single-utterance form is its batch row
        pair = torch.stack([mel, torch.from_numpy(R.mel_input(Tf, case["seed"] + 7))])
        assert torch.equal(gen.inference(pair)[0], got)


def test_ragged_rows_equal_the_single_runs_f16():
    gen, hop = _gen("v1_wn"), R.hop_of(R.CASES["v1_wn"]["cfg"])
    lengths = (13, 5, 1, 9)
    c = torch.full((4, 13, 80), float("nan"))
    for b, n in enumerate(lengths):
        c[b, :n] = torch.from_numpy(R.mel_input(n, 50 + b))
    y = gen.inference(c, lengths=lengths)
    assert y.shape == (4, 13 * hop, 1) and not bool(torch.isnan(y).any())
    for b, n in enumerate(lengths):
        alone = gen.inference(c[b, :n])
        assert torch.equal(y[b, :n * hop], alone), (b, float((y[b, :n * hop] - alone).abs().max()))
        assert not bool(y[b, n * hop:].any())
    full = torch.stack([torch.from_numpy(R.mel_input(13, 60 + b)) for b in range(3)])
    assert torch.equal(gen.inference(full, lengths=[13] * 3), gen.inference(full))


def test_span_window_reproduces_the_full_run_f16():
    from a3t_amd.vocoder import span_window
    gen, hop = _gen("v1_wn"), 300
    m = gen.margin_frames
    c = torch.from_numpy(R.mel_input(60, 9)).to(DEV)
    full = gen.inference(c)
    n0, n1 = 25, 28
    w0, w1 = span_window(n0, n1, 60, m)
    assert (w0, w1) == (n0 - m, n1 + m)
    win = gen.inference(c[w0:w1])
    assert torch.equal(win[(n0 - w0) * hop:(n1 - w0) * hop], full[n0 * hop:n1 * hop])
    rows = torch.zeros(2, w1 - w0, 80, device=DEV)
    rows[0], rows[1, :5] = c[w0:w1], c[:5]
    rag = gen.inference(rows, lengths=(w1 - w0, 5))
    assert torch.equal(rag[0, (n0 - w0) * hop:(n1 - w0) * hop], full[n0 * hop:n1 * hop])


def test_two_calls_give_the_same_bits_and_the_default_is_f32():
    c = torch.from_numpy(np.stack([R.mel_input(13, 3), R.mel_input(13, 4)])).to(DEV)
    keep = c.clone()
    gen = _gen("v1_wn")
    a, b = gen.inference(c), gen.inference(c)
    assert torch.equal(a, b) and torch.equal(c, keep)
    ar, br = gen.inference(c, lengths=[13, 6]), gen.inference(c, lengths=[13, 6])
    assert torch.equal(ar, br) and torch.equal(ar[0], a[0]) and torch.equal(c, keep)
    default, f32 = _gen("v1_wn", None), _gen("v1_wn", "f32")
    assert default.compute == f32.compute == "f32" and not any(st["f16"] for st in default.stages)
    d = default.inference(c)
    assert torch.equal(d, f32.inference(c)) and not torch.equal(d, a)
    assert float((d - a).abs().max()) < 1e-2      # (the same waveform, though)


def test_a_hot_input_gives_a_finite_waveform():
    """The mel scaled until a residual-block convolution's input exceeds 65504: the conversion saturates, no infinity is made."""
    case = R.CASES["v1_wn"]
    hot = torch.from_numpy(R.mel_input(2, 5)) * 1e5
    stats = {}
    H.generator(_state("v1_wn"), case["cfg"], hot, dtype=torch.float32, rnd_dtype=torch.float16, stats=stats)
    assert stats["max_in"] > 65504.0
    got = _gen("v1_wn").inference(hot)
    assert bool(torch.isfinite(got).all())


# --------------------------------------------------------------------------------------------------------- SpeechEditor
def test_speech_editor_span_only_equals_full_vocoding_f16():
    import test_gpu_sedit_batch as SB
    ed, oc, *_ = SB._editor()      # a fresh editor of our own (that helper is not cached)
    assert oc.hop_length == 300
    ed.vocoder = _gen("v1_wn")
    reqs = SB._requests()
    full = ed.edit_batch(reqs)
    span = ed.edit_batch(reqs, outputs=("orgin_replaced",))
    assert len(full) == len(span) == 4
    for f, s in zip(full, span):
        assert "prediction" not in s and "prediction" in f
        assert np.isfinite(f["prediction"]).all() and float(np.abs(f["prediction"]).max()) > 1e-3
        assert np.array_equal(f["orgin_replaced"], s["orgin_replaced"])
