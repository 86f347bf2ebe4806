"""Torch restatement of the HiFi-GAN generator (espnet2/gan_tts/hifigan/hifigan.py:25-221, residual_block.py:17-99) for the
tests of a3t_amd.vocoder.HiFiGANGeneratorHIP: the network in torch.nn.functional calls on a plain state dict, the ragged rule
of `lengths=`, the span-window arithmetic, procedural weights and seeded mels.  Shared by tests/golden/make_golden_hifigan.py
(which holds it against the reference's own module), tests/test_hifigan_host.py and tests/test_gpu_hifigan.py.

Ragged rule: row b of a padded batch is the row run alone.  Every convolution of stage i (rate_i = product of the scales so
far), the input convolution at frame rate and the output convolution read zeros at t >= lengths[b] * rate and store zeros
there (the biases would make padded positions non-zero otherwise)."""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

V1 = dict(in_channels=80, channels=512, kernel_size=7, upsample_scales=[5, 5, 4, 3], upsample_kernel_sizes=[10, 10, 8, 6],
          resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], use_additional_convs=True,
          bias=True, negative_slope=0.1)
# the reference constructor's own defaults (scales 8, 8, 2, 2) at an eighth of the width
DEFAULTS64 = dict(V1, channels=64, upsample_scales=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4])
ODD = dict(V1, channels=64, upsample_scales=[3, 2], upsample_kernel_sizes=[6, 4], resblock_kernel_sizes=[3, 5],
           resblock_dilations=[[1, 2], [2, 6]], use_additional_convs=False, bias=False)
CASES = {"v1_wn": dict(cfg=V1, weight_norm=True, seed=41), "defaults64": dict(cfg=DEFAULTS64, weight_norm=False, seed=42),
         "odd": dict(cfg=ODD, weight_norm=False, seed=43)}
FRAMES = (1, 2, 13)


def conv_names(cfg):
    """[(state-dict prefix, weight shape, has bias, gain)] of every convolution, in forward order.  The gains keep the signal
    alive and unsaturated under oracle.procedural_state's variance-preserving uniform weights: a convolution behind a LeakyReLU
    gets back what the activation takes (sqrt(2 / (1 + slope^2))); a transposed convolution, whose fan-in is two taps and not the
    2s * Cout procedural_state counts, sqrt(s * Cout / Cin) on top; the last convolution of every residual unit 0.5, so that three
    units grow the variance by about 2 and not by 8; the output convolution 0.5, which keeps tanh off its rails."""
    C, K, A = cfg["channels"], cfg["kernel_size"], cfg["in_channels"]
    g = math.sqrt(2.0 / (1.0 + cfg["negative_slope"] ** 2))
    out = [("input_conv", (C, A, K), True, 1.0)]
    nb = len(cfg["resblock_kernel_sizes"])
    for i, s in enumerate(cfg["upsample_scales"]):
        ci, co = C >> i, C >> (i + 1)
        out.append((f"upsamples.{i}.1", (ci, co, 2 * s), True, g * math.sqrt(s * co / ci)))
        for j, (k, dils) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilations"])):
            for d in range(len(dils)):
                p = f"blocks.{i * nb + j}."
                if cfg["use_additional_convs"]:
                    out.append((p + f"convs1.{d}.1", (co, co, k), cfg["bias"], g))
                    out.append((p + f"convs2.{d}.1", (co, co, k), cfg["bias"], 0.5 * g))
                else:
                    out.append((p + f"convs1.{d}.1", (co, co, k), cfg["bias"], 0.5 * g))
    out.append(("output_conv.1", (1, C >> len(cfg["upsample_scales"]), K), True, 0.5))
    return out


def procedural_hifigan_state(cfg, seed, weight_norm=False):
    """Deterministic weights of the generator as numpy arrays under the reference's state-dict keys.  weight_norm: weight_g /
    weight_v as torch.nn.utils.weight_norm stores them, v procedural and g = gain * ||v|| * (1 + 0.2 u), u uniform in (-1, 1), so
    that the folded weight is not v itself."""
    from oracle.a3t_oracle import procedural_state
    shapes = {}
    for p, shp, has_b, _ in conv_names(cfg):
        if weight_norm:
            shapes[p + ".weight_v"], shapes[p + ".weight_g"] = shp, (shp[0], 1, 1)
        else:
            shapes[p + ".weight"] = shp
        if has_b:
            shapes[p + ".bias"] = (shp[1] if p.startswith("upsamples") else shp[0],)
    st = procedural_state(shapes, seed)
    for p, shp, _, gain in conv_names(cfg):
        if weight_norm:
            v = st[p + ".weight_v"].astype(np.float64)
            n = np.sqrt((v.reshape(shp[0], -1) ** 2).sum(1)).reshape(-1, 1, 1)
            u = st[p + ".weight_g"].astype(np.float64) / math.sqrt(3.0)
            st[p + ".weight_g"] = (gain * n * (1.0 + 0.2 * u)).astype(np.float32)
        else:
            st[p + ".weight"] = (st[p + ".weight"] * np.float32(gain)).astype(np.float32)
    return st


def mel_input(T, seed, channels=80):
    """A seeded normalised-mel-like input [T][channels] fp32."""
    return np.random.RandomState(1000 + seed).standard_normal((T, channels)).astype(np.float32)


def folded(state, dtype=torch.float64):
    """{prefix.weight / prefix.bias: tensor of dtype}: weight norm folded in fp64 (w = g * v / ||v||, norm over all dims but 0)."""
    out = {}
    for k, v in state.items():
        t = torch.as_tensor(np.asarray(v))
        if k.endswith(".weight_v"):
            p = k[:-len(".weight_v")]
            v64, g64 = t.double(), torch.as_tensor(np.asarray(state[p + ".weight_g"])).double()
            out[p + ".weight"] = (g64 * v64 / v64.flatten(1).norm(dim=1).reshape(-1, 1, 1)).to(dtype)
        elif not k.endswith(".weight_g"):
            out[k] = t.to(dtype)
    return out


def generator(state, cfg, c, lengths=None, dtype=torch.float64, stages=None):
    """c [B][T][in_channels] (or [T][in_channels]) -> [B][T*hop][1] (or [T*hop][1]) in `dtype`, with the ragged rule when
    lengths (one per row) is given.  stages: a list that receives the RMS of the input convolution's, every stage's and the
    output's tensor."""
    w = folded(state, dtype)
    single = c.dim() == 2
    x = torch.as_tensor(c).to(dtype)
    x = (x[None] if single else x).transpose(1, 2).clone()             # [B][C][T]
    slope, K, nb = cfg["negative_slope"], cfg["kernel_size"], len(cfg["resblock_kernel_sizes"])

    def cut(x, rate):
        if lengths is not None:
            for b, n in enumerate(lengths):
                x[b, :, int(n) * rate:] = 0
        return x

    def rms(x):
        if stages is not None:
            stages.append(float(x.double().pow(2).mean().sqrt()))

    x = cut(x, 1)
    x = cut(F.conv1d(x, w["input_conv.weight"], w["input_conv.bias"], padding=(K - 1) // 2), 1)
    rms(x)
    rate = 1
    for i, s in enumerate(cfg["upsample_scales"]):
        rate *= s
        x = cut(F.conv_transpose1d(F.leaky_relu(x, slope), w[f"upsamples.{i}.1.weight"], w[f"upsamples.{i}.1.bias"], stride=s,
                                   padding=s // 2 + s % 2, output_padding=s % 2), rate)
        cs = None
        for j, (k, dils) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilations"])):
            p, y = f"blocks.{i * nb + j}.", x
            for d, dil in enumerate(dils):
                xt = cut(F.conv1d(F.leaky_relu(y, slope), w[p + f"convs1.{d}.1.weight"], w.get(p + f"convs1.{d}.1.bias"),
                                  padding=(k - 1) // 2 * dil, dilation=dil), rate)
                if cfg["use_additional_convs"]:
                    xt = cut(F.conv1d(F.leaky_relu(xt, slope), w[p + f"convs2.{d}.1.weight"], w.get(p + f"convs2.{d}.1.bias"),
                                      padding=(k - 1) // 2), rate)
                y = xt + y
            cs = y if cs is None else cs + y
        x = cs / nb
        rms(x)
    x = torch.tanh(F.conv1d(F.leaky_relu(x, 0.01), w["output_conv.1.weight"], w["output_conv.1.bias"], padding=(K - 1) // 2))
    x = cut(x, rate).transpose(1, 2)
    rms(x)
    return x[0] if single else x


def hop_of(cfg):
    return int(np.prod(cfg["upsample_scales"]))


def window(n0, n1, T, margin):
    """Frame window [w0, w1) to vocode for span [n0, n1) of a T-frame mel: span +- margin clipped to the mel."""
    return max(0, n0 - margin), min(T, n1 + margin)


def window_run(run, c, n0, n1, margin, hop):
    """The samples of span [n0, n1) from a run over the window only; run: mel [T'][A] -> [T'*hop][1]."""
    w0, w1 = window(n0, n1, c.shape[0], margin)
    y = run(c[w0:w1])
    return y[(n0 - w0) * hop:(n1 - w0) * hop]


def scale_of(a):
    return max(1.0, float(np.abs(np.asarray(a)).max()))


def bound(Fl, scale=1.0):
    """The tolerance of every comparison against an fp64 result: 4 x the loss F of an fp32 evaluation against fp64 on the same
    input (relative to scale), F floored at 1e-6: both sides are fp32 evaluations of the same sums in different orders, and the
    comparison takes the worst of several thousand samples."""
    return 4.0 * max(float(Fl), 1e-6) * scale
