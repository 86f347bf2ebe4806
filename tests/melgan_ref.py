"""Torch restatement of the MelGAN / multi-band MelGAN generator (espnet2/gan_tts/melgan/melgan.py:22-199,
residual_stack.py:16-71, pqmf.py:56-160) for the tests of a3t_amd.vocoder.MelGANGeneratorHIP: the network in
torch.nn.functional calls on a plain state dict, the ragged rule of `lengths=`, procedural weights and seeded mels.  Shared by
tests/golden/make_golden_melgan.py (which holds it against the reference's own modules), tests/test_melgan_host.py and
tests/test_gpu_melgan.py.

Ragged rule: row b of a padded batch is the row run alone.  Every reflection happens at the row's own ends at that layer's rate
(a tap at ts < 0 reads -ts, one at ts >= W_b reads 2 (W_b - 1) - ts), the transposed convolutions and the PQMF filter read zeros
beyond W_b, and the output is zero behind lengths[b] * hop.  The restatement does just that: it runs every row alone.

The PQMF synthesis filter is taken as fp32 values (the reference holds it as an fp32 buffer, and its .double() model computes with
those rounded values), also in the fp64 runs."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hifigan_ref import bound, mel_input, scale_of, window, window_run      # noqa: E402,F401  (one rule for every generator)

PQMF_V2 = dict(taps=62, cutoff_ratio=0.142, beta=9.0)
V2 = dict(in_channels=80, out_channels=4, kernel_size=7, channels=384, upsample_scales=[5, 5, 3], stack_kernel_size=3, stacks=4,
          bias=True, negative_slope=0.2, use_final_nonlinear_activation=True)
PLAIN_SMALL = dict(V2, out_channels=1, channels=64, upsample_scales=[4, 2], stacks=2, kernel_size=5,
                   use_final_nonlinear_activation=False)
ODD = dict(V2, channels=96, upsample_scales=[3, 5], stacks=3, bias=False)
CASES = {"mb_v2_wn": dict(cfg=V2, pqmf=PQMF_V2, weight_norm=True, seed=51, frames=(6, 7, 19)),
         "plain_small": dict(cfg=PLAIN_SMALL, pqmf=None, weight_norm=False, seed=52, frames=(3, 4, 13)),
         "odd": dict(cfg=ODD, pqmf=dict(taps=30, cutoff_ratio=0.15, beta=8.0), weight_norm=False, seed=53, frames=(4, 5, 13))}


def layer_index(cfg):
    """Indices into the reference's Sequential: (input conv, [(transposed conv, [stacks])] per stage, output conv)."""
    idx, stages = 2, []
    for _ in cfg["upsample_scales"]:
        stages.append((idx + 1, [idx + 2 + j for j in range(cfg["stacks"])]))
        idx += 2 + cfg["stacks"]
    return 1, stages, idx + 2


def conv_names(cfg):
    """[(state-dict prefix, weight shape, has bias)] of every convolution, in forward order."""
    C, K, A, ks = cfg["channels"], cfg["kernel_size"], cfg["in_channels"], cfg["stack_kernel_size"]
    i_in, stages, i_out = layer_index(cfg)
    out = [(f"melgan.{i_in}", (C, A, K))]
    for i, (s, (i_up, i_st)) in enumerate(zip(cfg["upsample_scales"], stages)):
        ci, co = C >> i, C >> (i + 1)
        out.append((f"melgan.{i_up}", (ci, co, 2 * s)))
        for j in i_st:
            out += [(f"melgan.{j}.stack.2", (co, co, ks)), (f"melgan.{j}.stack.4", (co, co, 1)),
                    (f"melgan.{j}.skip_layer", (co, co, 1))]
    out.append((f"melgan.{i_out}", (cfg["out_channels"], C >> len(cfg["upsample_scales"]), K)))
    return [(p, shp, cfg["bias"]) for p, shp in out]


def procedural_melgan_state(cfg, seed, weight_norm=False):
    """Deterministic weights of the generator as numpy arrays under the reference's state-dict keys: oracle.procedural_state's
    uniform +-sqrt(3 / fan_in), no gain (a gain of 1.4 already saturates every output sample).  weight_norm: weight_g / weight_v
    as torch.nn.utils.weight_norm stores them, v procedural and g = ||v|| * (1 + 0.2 u), u uniform in (-1, 1), so that the folded
    weight is not v itself."""
    from oracle.a3t_oracle import procedural_state
    shapes = {}
    for p, shp, has_b in conv_names(cfg):
        if weight_norm:
            shapes[p + ".weight_v"], shapes[p + ".weight_g"] = shp, (shp[0], 1, 1)
        else:
            shapes[p + ".weight"] = shp
        if has_b:
            shapes[p + ".bias"] = (shp[1] if p in _transposed(cfg) else shp[0],)      # (ConvTranspose1d: [Cin][Cout][k])
    st = procedural_state(shapes, seed)
    if weight_norm:
        for p, shp, _ in conv_names(cfg):
            v = st[p + ".weight_v"].astype(np.float64)
            n = np.sqrt((v.reshape(shp[0], -1) ** 2).sum(1)).reshape(-1, 1, 1)
            u = st[p + ".weight_g"].astype(np.float64) / np.sqrt(3.0)
            st[p + ".weight_g"] = (n * (1.0 + 0.2 * u)).astype(np.float32)
    return st


def _transposed(cfg):
    return {f"melgan.{i_up}" for i_up, _ in layer_index(cfg)[1]}


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


def pqmf_filter(subbands, taps=62, cutoff_ratio=0.142, beta=9.0):
    """The reference's synthesis filters [subbands][taps + 1] restated in numpy (np.kaiser), rounded to fp32."""
    n = np.arange(taps + 1) - 0.5 * taps
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.sin(np.pi * cutoff_ratio * n) / (np.pi * n)
    h[taps // 2] = np.cos(0) * cutoff_ratio
    h = h * np.kaiser(taps + 1, beta)
    out = np.zeros((subbands, taps + 1))
    for k in range(subbands):
        out[k] = 2 * h * np.cos((2 * k + 1) * (np.pi / (2 * subbands)) * (np.arange(taps + 1) - (taps / 2)) - (-1) ** k * np.pi / 4)
    return out.astype(np.float32)


def pqmf_synthesis(x, h):
    """x [B][S][Ts] -> [B][1][Ts * S] with the fp32 filter h [S][taps + 1], in x's dtype: the reference's zero-stuffing transposed
    convolution (times S), zero padding and convolution."""
    S, taps = h.shape[0], h.shape[1] - 1
    up = torch.zeros(S, S, S, dtype=x.dtype)
    for k in range(S):
        up[k, k, 0] = 1.0
    y = F.conv_transpose1d(x, up * S, stride=S)
    return F.conv1d(F.pad(y, (taps // 2, taps // 2)), torch.as_tensor(h).to(x.dtype)[None])


def _row(w, cfg, pq, x, stages):
    """One row [1][A][T] -> [1][1][T * hop]."""
    slope, K, ks = cfg["negative_slope"], cfg["kernel_size"], cfg["stack_kernel_size"]
    i_in, st, i_out = layer_index(cfg)
    half = (K - 1) // 2

    def rms(x):
        if stages is not None:
            stages.append(float(x.double().pow(2).mean().sqrt()))

    x = F.conv1d(F.pad(x, (half, half), mode="reflect"), w[f"melgan.{i_in}.weight"], w.get(f"melgan.{i_in}.bias"))
    rms(x)
    for s, (i_up, i_st) in zip(cfg["upsample_scales"], st):
        x = F.conv_transpose1d(F.leaky_relu(x, slope), w[f"melgan.{i_up}.weight"], w.get(f"melgan.{i_up}.bias"), stride=s,
                               padding=s // 2 + s % 2, output_padding=s % 2)
        for j, i in enumerate(i_st):
            p, d = f"melgan.{i}.", ks ** j
            pad = (ks - 1) // 2 * d
            h = F.conv1d(F.pad(F.leaky_relu(x, slope), (pad, pad), mode="reflect"), w[p + "stack.2.weight"], w.get(p + "stack.2.bias"),
                         dilation=d)
            h = F.conv1d(F.leaky_relu(h, slope), w[p + "stack.4.weight"], w.get(p + "stack.4.bias"))
            x = h + F.conv1d(x, w[p + "skip_layer.weight"], w.get(p + "skip_layer.bias"))
        rms(x)
    x = F.conv1d(F.pad(F.leaky_relu(x, slope), (half, half), mode="reflect"), w[f"melgan.{i_out}.weight"], w.get(f"melgan.{i_out}.bias"))
    if cfg["use_final_nonlinear_activation"]:
        x = torch.tanh(x)
    rms(x)
    if cfg["out_channels"] > 1:
        x = pqmf_synthesis(x, pqmf_filter(cfg["out_channels"], **pq))
        rms(x)
    return x


def generator(state, cfg, c, pqmf=None, lengths=None, dtype=torch.float64, stages=None):
    """c [B][T][in_channels] (or [T][in_channels]) -> [B][T*hop][1] (or [T*hop][1]) in `dtype`, with the ragged rule when lengths
    (one per row) is given.  stages: a list that receives the RMS of the input convolution's, every stage's, the output
    convolution's and (multi-band) the PQMF's tensor (of the last row)."""
    w = folded(state, dtype)
    single = c.dim() == 2
    x = torch.as_tensor(c).to(dtype)
    x = x[None] if single else x
    B, T, _ = x.shape
    hop = hop_of(cfg)
    out = torch.zeros(B, T * hop, 1, dtype=dtype)
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        if n:
            if stages is not None:
                del stages[:]
            out[b, :n * hop, 0] = _row(w, cfg, pqmf or PQMF_V2, x[b:b + 1, :n].transpose(1, 2), stages)[0, 0]
    return out[0] if single else out


def hop_of(cfg):
    return int(np.prod(cfg["upsample_scales"])) * cfg["out_channels"]
