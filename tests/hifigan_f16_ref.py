"""CPU restatement of the HiFi-GAN generator with reduced-precision operands in the residual-block convolutions: the yardstick
of HiFiGANGeneratorHIP(compute="f16") (a3t_amd/csrc/hifigan_f16.hip).

It is hifigan_ref.generator, statement for statement, with an optional rounding dtype applied at exactly two points of every
residual-block convolution (convs1 and convs2):
  1. its input leaky(x, slope): computed in fp32 (x and the product x * slope as fp32, like the kernel), rounded, then cast to
     the accumulation dtype;
  2. its weight: folded in fp64, cast to fp32 (what the host class holds), rounded, then cast to the accumulation dtype.
Rounding is round-to-nearest-even to the dtype (torch's cast) after saturation to +-65504 for fp16 (pwg_f16_ref.rounder).
Everything else stays in the accumulation dtype (float64 or float32): sums, biases, residuals, the MRF mean, the input, transposed
and output convolutions.  With rounding off it is hifigan_ref.generator bit for bit.
Not a test module: tests/test_hifigan_f16_host.py and tests/test_gpu_hifigan_f16.py import it."""
import numpy as np
import torch
import torch.nn.functional as F

import hifigan_ref as R
from pwg_f16_ref import errors, rounder      # noqa: F401  (errors: re-exported for the tests)


def _operands(y, w, slope, rnd_dtype, dtype):
    """(conv input, weight) of one residual-block convolution in `dtype`, rounded to rnd_dtype (None: not at all)."""
    if rnd_dtype is None:
        return F.leaky_relu(y, slope), w
    rnd = rounder(rnd_dtype)
    return rnd(F.leaky_relu(y.to(torch.float32), slope)).to(dtype), rnd(w.to(torch.float32)).to(dtype)


def generator(state, cfg, c, lengths=None, dtype=torch.float64, rnd_dtype=None, stats=None):
    """hifigan_ref.generator with the two rounding points.  stats (a dict): "max_in" receives the largest |leaky(x)| that reaches
    a residual-block convolution, before rounding."""
    w = R.folded(state, dtype)
    single = c.dim() == 2
    x = torch.as_tensor(c).to(dtype)
    x = (x[None] if single else x).transpose(1, 2).clone()             # [B][C][T]
    slope, K, nb = cfg["negative_slope"], cfg["kernel_size"], len(cfg["resblock_kernel_sizes"])

    def cut(x, rate):
        if lengths is not None:
            for b, n in enumerate(lengths):
                x[b, :, int(n) * rate:] = 0
        return x

    def conv(y, name, pad, dil):
        a, wt = _operands(y, w[name + ".weight"], slope, rnd_dtype, dtype)
        if stats is not None:
            stats["max_in"] = max(stats.get("max_in", 0.0), float(F.leaky_relu(y, slope).abs().max()))
        return F.conv1d(a, wt, w.get(name + ".bias"), padding=pad, dilation=dil)

    x = cut(x, 1)
    x = cut(F.conv1d(x, w["input_conv.weight"], w["input_conv.bias"], padding=(K - 1) // 2), 1)
    rate = 1
    for i, s in enumerate(cfg["upsample_scales"]):
        rate *= s
        x = cut(F.conv_transpose1d(F.leaky_relu(x, slope), w[f"upsamples.{i}.1.weight"], w[f"upsamples.{i}.1.bias"], stride=s,
                                   padding=s // 2 + s % 2, output_padding=s % 2), rate)
        cs = None
        for j, (k, dils) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilations"])):
            p, y = f"blocks.{i * nb + j}.", x
            for d, dil in enumerate(dils):
                xt = cut(conv(y, p + f"convs1.{d}.1", (k - 1) // 2 * dil, dil), rate)
                if cfg["use_additional_convs"]:
                    xt = cut(conv(xt, p + f"convs2.{d}.1", (k - 1) // 2, 1), rate)
                y = xt + y
            cs = y if cs is None else cs + y
        x = cs / nb
    x = torch.tanh(F.conv1d(F.leaky_relu(x, 0.01), w["output_conv.1.weight"], w["output_conv.1.bias"], padding=(K - 1) // 2))
    x = cut(x, rate).transpose(1, 2)
    return x[0] if single else x


def conv_unit(x, w, bias, dil, slope, rnd_dtype=None, dtype=torch.float64, res=None, acc0=None, alpha=1.0, acc_add=False):
    """One convolution with the kernel's epilogue forms on one row alone: x [n][C] fp32, w [C][C][k] fp32, bias [C] or None ->
    (v, acc) in `dtype`: v = bias + conv(leaky(x)) (+ res), acc = alpha * v, or acc0 + alpha * v with acc_add."""
    a, wt = _operands(x.t()[None].to(torch.float32 if rnd_dtype is not None else dtype), w.to(dtype), slope, rnd_dtype, dtype)
    k = w.shape[2]
    v = F.conv1d(a.to(dtype), wt, None if bias is None else bias.to(dtype), padding=(k - 1) // 2 * dil, dilation=dil)[0].t()
    if res is not None:
        v = v + res.to(dtype)
    acc = alpha * v
    if acc_add:
        acc = acc0.to(dtype) + acc
    return v, acc


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2)))
