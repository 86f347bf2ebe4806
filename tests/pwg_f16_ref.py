"""CPU restatement of the ParallelWaveGAN generator with reduced-precision operands in the residual blocks: the yardstick of
ParallelWaveGANGeneratorHIP(compute="f16") (a3t_amd/csrc/pwg_fused_f16.hip).

It is the oracle's pwg_forward, statement for statement, with an optional rounding dtype applied at exactly these points:
  1. the input x of every block's dilated convolution;
  2. the upsampled conditioning cu;
  3. the gate output g;
  4. the three weight matrices of every block (conv, conv1x1_aux, conv1x1_out).
Rounding is round-to-nearest-even to the dtype (torch's cast) after saturation to +-65504 for fp16, and back to fp32.
Everything else stays fp32: accumulation, biases, tanh / sigmoid, the residual stream, skips, the upsampling network,
first_conv and the last two layers.  With rounding off it is pwg_forward bit for bit.
Not a test module: tests/test_vocoder_f16_host.py and tests/test_gpu_vocoder_f16.py import it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import a3t_oracle as O

F16_MAX = 65504.0


def rounder(dtype):
    """None -> identity; torch.float16 / torch.bfloat16 -> round to that dtype (fp16: saturated) and back to fp32."""
    if dtype is None:
        return lambda t: t
    if dtype == torch.float16:
        return lambda t: t.clamp(-F16_MAX, F16_MAX).to(torch.float16).to(torch.float32)
    return lambda t: t.to(dtype).to(torch.float32)


def vocoder_state(seed=4):
    """The tests' procedural generator weights: the smoothing filters of the upsampling network normalised to sum 1."""
    cfg = O.PWGConfig()
    state = O.procedural_state(O.pwg_param_shapes(cfg), seed=seed)
    for k in state:
        if "up_layers" in k:
            state[k] = np.abs(state[k]) / np.abs(state[k]).sum()
    return cfg, state


def table_inputs(T, B=2, seed=7, hop=300):
    """c ~ U(-4, 2) of shape (B, 80, T) and z ~ N(0, 1) of shape (B, 1, T * hop), drawn in this order from RandomState(seed)."""
    rs = np.random.RandomState(seed)
    c = rs.uniform(-4.0, 2.0, (B, 80, T)).astype(np.float32)
    z = rs.standard_normal((B, 1, T * hop)).astype(np.float32)
    return torch.from_numpy(c), torch.from_numpy(z)


def block(p, pre, x, c, dil, cfg, rnd):
    """One residual block: x (B, 64, T), c (B, 80, T) (already rounded where rounding applies) -> (x_out, skip contribution)."""
    y = F.conv1d(rnd(x), rnd(p[pre + "conv.weight"]), p[pre + "conv.bias"], padding=(cfg.kernel_size - 1) // 2 * dil, dilation=dil)
    xa, xb = y.split(y.shape[1] // 2, dim=1)
    ca, cb = F.conv1d(c, rnd(p[pre + "conv1x1_aux.weight"])).split(y.shape[1] // 2, dim=1)
    g = torch.tanh(xa + ca) * torch.sigmoid(xb + cb)
    o = F.conv1d(rnd(g), rnd(p[pre + "conv1x1_out.weight"]), p[pre + "conv1x1_out.bias"])
    r, s = o.split([cfg.res_ch, cfg.skip_ch], dim=1)
    return (r + x) * math.sqrt(0.5), s


@torch.no_grad()
def pwg_forward(p, c_feats, z, cfg, dtype=None, stats=None):
    """O.pwg_forward with the rounding points above.  c_feats (B, 80, T_feats), z (B, 1, T_wav) -> (B, 1, T_wav).
    stats (a dict): filled with the largest |x| and |cu| that reach a block ("max_x", "max_cu"), before rounding."""
    rnd = rounder(dtype)
    w = cfg.aux_context_window
    c = F.pad(c_feats, (w, w), mode="replicate")
    c = F.conv1d(c, p["upsample_net.conv_in.weight"])
    c = c.unsqueeze(1)
    for i, sc in enumerate(cfg.upsample_scales):
        c = F.interpolate(c, scale_factor=(1, sc), mode="nearest")
        c = F.conv2d(c, p[f"upsample_net.upsample.up_layers.{2 * i + 1}.weight"], padding=(0, sc))
    c = c.squeeze(1)
    c16 = rnd(c)
    x = F.conv1d(z, p["first_conv.weight"], p["first_conv.bias"])
    skips = 0
    lps = cfg.layers // cfg.stacks
    for l in range(cfg.layers):
        if stats is not None:
            stats["max_x"] = max(stats.get("max_x", 0.0), float(x.abs().max()))
            stats["max_cu"] = max(stats.get("max_cu", 0.0), float(c.abs().max()))
        x, s = block(p, f"conv_layers.{l}.", x, c16, 2 ** (l % lps), cfg, rnd)
        skips = skips + s
    skips = skips * math.sqrt(1.0 / cfg.layers)
    x = torch.relu(skips)
    x = torch.relu(F.conv1d(x, p["last_conv_layers.1.weight"], p["last_conv_layers.1.bias"]))
    return F.conv1d(x, p["last_conv_layers.3.weight"], p["last_conv_layers.3.bias"])


def errors(got, ref):
    """(RMS error / RMS of ref, worst element / max |ref|) of two arrays or tensors."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    d = got - ref
    return float(np.sqrt(np.mean(d * d)) / np.sqrt(np.mean(ref * ref))), float(np.abs(d).max() / np.abs(ref).max())
