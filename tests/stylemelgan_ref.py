"""Torch restatement of the StyleMelGAN generator (espnet2/gan_tts/style_melgan/style_melgan.py:28-232,
tade_res_block.py:15-185) for the tests of a3t_amd.vocoder.StyleMelGANGeneratorHIP: the network in torch.nn.functional calls on a
plain state dict, the ragged rule of `lengths=`, procedural weights, seeded mels and seeded noise.  Shared by
tests/golden/make_golden_stylemelgan.py (which holds it against the reference's own module), tests/test_stylemelgan_host.py and
tests/test_gpu_stylemelgan.py.

Row rule: row b of a padded batch is the row run alone by the reference's `inference` with the row's own noise: m_b = ceil(n_b / F)
noise steps (F = prod(noise_upsample_scales)), a network length of n_eff_b = m_b * F frames, c padded to it with the row's last
frame, zeros outside [0, n_eff_b * rate) for every convolution, every InstanceNorm statistic over the row's own n_eff_b * rate
samples, and an output that is zero behind n_b * hop.  The restatement does just that: it runs every row alone."""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hifigan_ref import bound, folded, mel_input, scale_of      # noqa: E402,F401  (one rule for every generator)

V1 = dict(in_channels=128, aux_channels=80, channels=64, out_channels=1, kernel_size=9, dilation=2, bias=True,
          noise_upsample_scales=[10, 2, 2, 2], noise_upsample_negative_slope=0.2, upsample_scales=[5, 1, 5, 1, 3, 1, 2, 2, 1],
          gated_function="softmax")
SMALL_SIGMOID = dict(V1, in_channels=16, aux_channels=16, kernel_size=5, dilation=3, noise_upsample_scales=[2, 2],
                     upsample_scales=[2, 1, 3], gated_function="sigmoid", bias=False)
ODD = dict(V1, in_channels=32, kernel_size=7, dilation=1, noise_upsample_scales=[3, 2], upsample_scales=[3, 2, 1])
# gate_gain: the factor on the gated_conv1 / gated_conv2 weights.  The plan amplifies rounding by an amount that grows with the
# sharpness of the gates: at gain 1 the reference's own fp32 run of the 9-block plan is 2.5e-4 of scale from its fp64
# run, at 0.5 between 2e-6 and 7e-5 depending on the seed and on the order of the fp32 sums (the threads of the CPU run), at 0.25
# it is 3e-7: v1_wn uses 0.25, where two fp32 evaluations agree well enough for a bound of 4 F to mean something.
CASES = {"v1_wn": dict(cfg=V1, weight_norm=True, seed=61, gate_gain=0.25, frames=(1, 81)),
         "small_sigmoid": dict(cfg=SMALL_SIGMOID, weight_norm=False, seed=62, gate_gain=1.0, frames=(1, 4, 5, 45)),
         "odd": dict(cfg=ODD, weight_norm=False, seed=63, gate_gain=1.0, frames=(2, 3, 4, 50))}


def hop_of(cfg):
    return int(np.prod(cfg["upsample_scales"]))


def noise_factor(cfg):
    return int(np.prod(cfg["noise_upsample_scales"]))


def noise_steps(cfg, frames):
    return -(-int(frames) // noise_factor(cfg))


def n_eff(cfg, frames):
    """The network length in frames of an input of `frames` frames."""
    return noise_steps(cfg, frames) * noise_factor(cfg)


def conv_names(cfg, gate_gain=1.0):
    """[(state-dict prefix, weight shape, transposed, gain)] of every convolution, in forward order."""
    C, K, A, Z = cfg["channels"], cfg["kernel_size"], cfg["aux_channels"], cfg["in_channels"]
    out = []
    for i, s in enumerate(cfg["noise_upsample_scales"]):
        out.append((f"noise_upsample.{2 * i}", (Z if i == 0 else C, C, 2 * s), True, 1.0))
    for k in range(len(cfg["upsample_scales"])):
        p = f"blocks.{k}."
        out += [(p + "tade1.aux_conv.0", (C, A if k == 0 else C, K), False, 1.0), (p + "tade1.gated_conv.0", (2 * C, C, K), False, 1.0),
                (p + "gated_conv1", (2 * C, C, K), False, gate_gain), (p + "tade2.aux_conv.0", (C, C, K), False, 1.0),
                (p + "tade2.gated_conv.0", (2 * C, C, K), False, 1.0), (p + "gated_conv2", (2 * C, C, K), False, gate_gain)]
    out.append(("output_conv.0", (cfg["out_channels"], C, K), False, 1.0))
    return out


def procedural_stylemelgan_state(cfg, seed, weight_norm=False, gate_gain=1.0):
    """Deterministic weights of the generator as numpy arrays under the reference's state-dict keys: oracle.procedural_state's
    uniform +-sqrt(3 / fan_in), the gated convolutions of the blocks times gate_gain.  weight_norm: weight_g / weight_v as
    torch.nn.utils.weight_norm stores them, v procedural and g = gain * ||v|| * (1 + 0.2 u), u uniform in (-1, 1), so that the
    folded weight is not v itself."""
    from oracle.a3t_oracle import procedural_state
    shapes = {}
    for p, shp, tr, _ in conv_names(cfg):
        if weight_norm:
            shapes[p + ".weight_v"], shapes[p + ".weight_g"] = shp, (shp[0], 1, 1)
        else:
            shapes[p + ".weight"] = shp
        if cfg["bias"]:
            shapes[p + ".bias"] = (shp[1] if tr else shp[0],)
    st = procedural_state(shapes, seed)
    for p, shp, _, gain in conv_names(cfg, gate_gain):
        if weight_norm:
            v = st[p + ".weight_v"].astype(np.float64)
            n = np.sqrt((v.reshape(shp[0], -1) ** 2).sum(1)).reshape(-1, 1, 1)
            u = st[p + ".weight_g"].astype(np.float64) / math.sqrt(3.0)
            st[p + ".weight_g"] = (gain * n * (1.0 + 0.2 * u)).astype(np.float32)
        elif gain != 1.0:
            st[p + ".weight"] = (st[p + ".weight"] * np.float32(gain)).astype(np.float32)
    return st


def case_state(name):
    case = CASES[name]
    return procedural_stylemelgan_state(case["cfg"], case["seed"], case["weight_norm"], case["gate_gain"])


def noise_input(cfg, frames, seed):
    """The seeded noise [ceil(frames / F)][in_channels] fp32 of an input of `frames` frames."""
    return np.random.RandomState(2000 + seed).standard_normal((noise_steps(cfg, frames), cfg["in_channels"])).astype(np.float32)


def _gate(cfg, v):
    xa, xb = v.split(v.size(1) // 2, dim=1)
    return (torch.softmax(xa, dim=1) if cfg["gated_function"] == "softmax" else torch.sigmoid(xa)) * torch.tanh(xb)


def _tade(w, p, K, x, c, u):
    """TADELayer: (x [1][C][T], c [1][A][T]) -> (y, c) at T * u."""
    x = F.instance_norm(x)
    c = F.conv1d(F.interpolate(c, scale_factor=u, mode="nearest"), w[p + "aux_conv.0.weight"], w.get(p + "aux_conv.0.bias"),
                 padding=(K - 1) // 2)
    cg1, cg2 = F.conv1d(c, w[p + "gated_conv.0.weight"], w.get(p + "gated_conv.0.bias"), padding=(K - 1) // 2).chunk(2, dim=1)
    return cg1 * F.interpolate(x, scale_factor=u, mode="nearest") + cg2, c


def block(w, cfg, k, x, c):
    """TADEResBlock k: (x [1][C][T], c [1][A][T]) -> (x, c) at T * upsample_scales[k]; w: folded(state)."""
    K, d, u, p = cfg["kernel_size"], cfg["dilation"], cfg["upsample_scales"][k], f"blocks.{k}."
    res = x
    x, c = _tade(w, p + "tade1.", K, x, c, 1)
    x = _gate(cfg, F.conv1d(x, w[p + "gated_conv1.weight"], w.get(p + "gated_conv1.bias"), padding=(K - 1) // 2))
    x, c = _tade(w, p + "tade2.", K, x, c, u)
    x = _gate(cfg, F.conv1d(x, w[p + "gated_conv2.weight"], w.get(p + "gated_conv2.bias"), padding=(K - 1) // 2 * d, dilation=d))
    return F.interpolate(res, scale_factor=u, mode="nearest") + x, c


def _row(w, cfg, c, z, blocks):
    """One row: c [1][A][n], z [1][Z][m] -> [1][1][n * hop].  blocks: a list that receives (x_in, c_in, x_out, c_out) of every
    block, each [T][C]."""
    n = c.shape[2]
    x = z
    for i, s in enumerate(cfg["noise_upsample_scales"]):
        p = f"noise_upsample.{2 * i}."
        x = F.leaky_relu(F.conv_transpose1d(x, w[p + "weight"], w.get(p + "bias"), stride=s, padding=s // 2 + s % 2,
                                            output_padding=s % 2), cfg["noise_upsample_negative_slope"])
    c = F.pad(c, (0, x.shape[2] - n), mode="replicate")
    for k in range(len(cfg["upsample_scales"])):
        xi, ci = x, c
        x, c = block(w, cfg, k, x, c)
        if blocks is not None:
            blocks.append(tuple(t[0].t().contiguous() for t in (xi, ci, x, c)))
    K = cfg["kernel_size"]
    x = torch.tanh(F.conv1d(x, w["output_conv.0.weight"], w.get("output_conv.0.bias"), padding=(K - 1) // 2))
    return x[..., :n * hop_of(cfg)]


def generator(state, cfg, c, z, lengths=None, dtype=torch.float64, blocks=None):
    """c [B][T][aux] (or [T][aux]), z [B][ceil(T / F)][in] (or [ceil(T / F)][in]) -> [B][T*hop][1] (or [T*hop][1]) in `dtype`, with
    the row rule when lengths (one per row) is given: row b uses z[b, :ceil(lengths[b] / F)].  blocks: a list that receives the
    block tensors of the last row (see _row)."""
    w = folded(state, dtype)
    single = c.dim() == 2
    x, zz = torch.as_tensor(c).to(dtype), torch.as_tensor(z).to(dtype)
    if single:
        x, zz = x[None], zz[None]
    B, T, _ = x.shape
    hop = hop_of(cfg)
    out = torch.zeros(B, T * hop, 1, dtype=dtype)
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        if n:
            if blocks is not None:
                del blocks[:]
            out[b, :n * hop, 0] = _row(w, cfg, x[b:b + 1, :n].transpose(1, 2), zz[b:b + 1, :noise_steps(cfg, n)].transpose(1, 2),
                                       blocks)[0, 0]
    return out[0] if single else out
