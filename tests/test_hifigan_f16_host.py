"""HiFiGANGeneratorHIP(compute="f16") on the host: the restatement tests/hifigan_f16_ref.py, the weight packing of
a3t_hfg_conv_f16, the constructor's refusals and what the fp16 operands cost against the fp64 outputs of the reference
(tests/golden/hifigan.npz).  No device needed.

Measured loss of the restatement (fp16 / bf16 operands in the residual-block convolutions, fp32 accumulation) against the fp64
golden outputs at 13 frames, RMS / RMS(ref) and worst element / max|ref| (procedural weights; trained checkpoints were not
available):
    plan         fp16                   bf16
    v1_wn        5.48e-4 / 9.60e-4      4.47e-3 / 8.90e-3
    defaults64   8.14e-4 / 1.14e-3      6.31e-3 / 9.72e-3
    odd          1.61e-4 / 2.47e-4      1.29e-3 / 2.10e-3
The test's bound is 2 x the fp16 column (the headroom of test_vocoder_f16_host.py)."""
import functools
import os

import numpy as np
import pytest
import torch

import hifigan_ref as R
import hifigan_f16_ref as H

G = os.path.join(os.path.dirname(__file__), "golden")
# (RMS / RMS ref, worst / max|ref|) of the fp16 restatement at 13 frames, measured with this file's _loss
F16_LOSS = {"v1_wn": (5.48e-4, 9.60e-4), "defaults64": (8.14e-4, 1.14e-3), "odd": (1.61e-4, 2.47e-4)}


@functools.lru_cache(maxsize=None)
def _state(name):
    c = R.CASES[name]
    return R.procedural_hifigan_state(c["cfg"], c["seed"], c["weight_norm"])


@functools.lru_cache(maxsize=None)
def _loss(name, rnd_dtype, Tf=13):
    case = R.CASES[name]
    want = np.load(os.path.join(G, "hifigan.npz"))[f"{name}.T{Tf}.wav64"]
    got = H.generator(_state(name), case["cfg"], torch.from_numpy(R.mel_input(Tf, case["seed"])), dtype=torch.float32,
                      rnd_dtype=rnd_dtype)
    return H.errors(got.numpy(), want)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_without_rounding_is_the_reference_restatement(name, dtype):
    case = R.CASES[name]
    c = torch.from_numpy(np.stack([R.mel_input(13, case["seed"]), R.mel_input(13, case["seed"] + 1)]))
    for lengths in (None, (13, 5)):
        a = H.generator(_state(name), case["cfg"], c, lengths=lengths, dtype=dtype)
        b = R.generator(_state(name), case["cfg"], c, lengths=lengths, dtype=dtype)
        assert a.dtype == dtype and torch.equal(a, b)
    assert torch.equal(H.generator(_state(name), case["cfg"], c[0], dtype=dtype), R.generator(_state(name), case["cfg"], c[0], dtype=dtype))


@pytest.mark.parametrize("C,k", [(32, 3), (64, 7), (128, 11), (256, 3)])
def test_pack_follows_its_index_formula(C, k):
    from a3t_amd.vocoder import pack_hifigan_conv_f16
    g = torch.Generator().manual_seed(C + k)
    w = torch.randn(C, C, k, generator=g)
    w[0, 0, 0], w[1, 0, 0], w[2, 0, 0] = 1e6, -1e6, 65519.0      # saturated, not inf
    P = pack_hifigan_conv_f16(w)
    assert P.dtype == torch.float16 and P.is_contiguous() and tuple(P.shape) == (k * C // 16, C // 32, 64, 8)
    w16 = H.rounder(torch.float16)(w)
    assert float(w16[0, 0, 0]) == 65504.0 and float(w16[1, 0, 0]) == -65504.0 and float(w16[2, 0, 0]) == 65504.0
    ks, mt, l, j = torch.meshgrid(torch.arange(P.shape[0]), torch.arange(C // 32), torch.arange(64), torch.arange(8), indexing="ij")
    want = w16[32 * mt + (l & 31), 16 * (ks % (C // 16)) + 8 * (l >> 5) + j, ks // (C // 16)]
    assert torch.equal(P.float(), want)
    # un-permuted, it is the rounded weight: every element is there exactly once
    back = torch.zeros(C, C, k)
    back[32 * mt + (l & 31), 16 * (ks % (C // 16)) + 8 * (l >> 5) + j, ks // (C // 16)] = P.float()
    assert torch.equal(back, w16)
    with pytest.raises(ValueError):
        pack_hifigan_conv_f16(torch.zeros(48, 48, 3))
    with pytest.raises(ValueError):
        pack_hifigan_conv_f16(torch.zeros(64, 32, 3))


def test_constructor_refusals_and_f16_stages():
    from a3t_amd import _lib
    from a3t_amd.vocoder import F16_WIDTHS, HiFiGANGeneratorHIP
    assert "a3t_hfg_conv_f16" in _lib.EXPORTS and len(_lib._SIGS["a3t_hfg_conv_f16"]) == len(_lib._SIGS["a3t_hfg_conv"])
    assert set(F16_WIDTHS) <= {32, 64, 128, 256}
    cfg = R.CASES["v1_wn"]["cfg"]
    # refused before the state dict or the device is looked at
    with pytest.raises(ValueError, match="compute"):
        HiFiGANGeneratorHIP({}, device="no-such-device", compute="bf16", **cfg)
    with pytest.raises(ValueError, match="fused"):
        HiFiGANGeneratorHIP({}, device="no-such-device", compute="f16", fused=False, **cfg)
    for name in R.CASES:
        cfg = R.CASES[name]["cfg"]
        gen = HiFiGANGeneratorHIP(_state(name), device="cpu", compute="f16", **cfg)
        ref = HiFiGANGeneratorHIP(_state(name), device="cpu", **cfg)
        assert gen.compute == "f16" and ref.compute == "f32" and gen.fused and gen.margin_frames == ref.margin_frames
        for st, st32 in zip(gen.stages, ref.stages):
            f16 = st["C"] in F16_WIDTHS
            assert st["f16"] == f16 and not st32["f16"] and st["fused"] == (f16 or st32["fused"])
            for blk, blk32 in zip(st["blocks"], st32["blocks"]):
                for u, u32 in zip(blk["units"], blk32["units"]):
                    for wt, wt32 in zip(u["w"], u32["w"]):
                        assert wt.dtype == (torch.float16 if f16 else torch.float32)
                        if not f16:
                            assert torch.equal(wt, wt32)
    params = {k: v for k, v in R.CASES["v1_wn"]["cfg"].items() if k != "negative_slope"}
    params["nonlinear_activation_params"] = dict(negative_slope=0.1)
    gen = HiFiGANGeneratorHIP.from_config(_state("v1_wn"), params, device="cpu", compute="f16")
    assert gen.compute == "f16" and all(st["f16"] for st in gen.stages)


@pytest.mark.parametrize("name", list(R.CASES))
def test_fp16_operands_cost_what_was_measured_and_less_than_bf16(name):
    f16, bf16 = _loss(name, torch.float16), _loss(name, torch.bfloat16)
    f32 = _loss(name, None)
    print(f"{name} T=13 against fp64: fp32 {f32[0]:.2e} / {f32[1]:.2e}, fp16 operands {f16[0]:.2e} / {f16[1]:.2e}, "
          f"bf16 operands {bf16[0]:.2e} / {bf16[1]:.2e}")
    assert f16[0] <= 2 * F16_LOSS[name][0] and f16[1] <= 2 * F16_LOSS[name][1]
    assert bf16[0] > f16[0] and bf16[1] > f16[1]
    assert f32[0] < f16[0] and f32[1] < f16[1]      # the rounding is what is being measured
