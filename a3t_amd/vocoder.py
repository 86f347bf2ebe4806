"""ParallelWaveGAN generator inference on the GPU (mel -> waveform).

Mirror of the vocoder the reference calls in ``sedit_inference.py:77,339-348`` through
``ParallelWaveGANPretrainedVocoder`` (espnet2/tts/utils/parallel_wavegan_pretrained_vocoder.py:49-63);
the network restated is the vendored twin ``ParallelWaveGANGenerator``
(espnet2/gan_tts/parallel_wavegan/parallel_wavegan.py:136-229, wavenet/residual_block.py:114-169,
parallel_wavegan/upsample.py:22-189), weight-norm removed.  Layout is channels-last [T][C] so every
Conv1d (dilated k=3, 1x1) is the shared implicit-im2col MFMA GEMM; the gated activation, residual /
skip update and nearest-neighbour upsampling+smoothing are element-wise HIP kernels.

HiFiGANGeneratorHIP (below) is the second generator family of the same model zoo, with the same inference interface.
"""
import math
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import ACT_RELU, ACT_TANH, F32


def pwg_margin_frames(layers=30, stacks=3, kernel_size=3, upsample_scales: Sequence[int] = (4, 5, 3, 5),
                      aux_context_window=2) -> int:
    """How many mel frames to each side of a frame span the generator's output inside the span depends on.  The residual
    stack (`stacks` x dilations 1 .. 2^(layers/stacks - 1), kernel k) reaches R = stacks * (2^(layers/stacks) - 1) * (k - 1) / 2
    samples, the smoothing convolution of upsampling stage i (2 * scale_i + 1 taps at its own rate) scale_i * prod_{j>i} scale_j
    samples, conv_in another aux_context_window frames: ceil((R + U) / hop) + aux_context_window.  14 for the v1 plan."""
    scales = [int(x) for x in upsample_scales]
    hop = int(np.prod(scales))
    R = stacks * (2 ** (layers // stacks) - 1) * (kernel_size - 1) // 2
    U = sum(sc * int(np.prod(scales[i + 1:])) for i, sc in enumerate(scales))
    return -(-(R + U) // hop) + int(aux_context_window)


def span_window(n0: int, n1: int, T: int, margin: int):
    """Frame window [w0, w1) that has to be vocoded so that the samples of span [n0, n1) of a T-frame utterance come out as in
    a run over the whole utterance: span +- margin, clipped to the utterance (where it is clipped the window's edge IS the
    utterance's edge and the generator's edge rules are the right ones)."""
    n0, n1 = max(0, min(int(n0), T)), max(0, min(int(n1), T))
    return max(0, n0 - margin), min(T, max(n1, n0) + margin)


def pwg_tile_list(lengths: Sequence[int], hop: int, tile: int = 256) -> np.ndarray:
    """The work list of a3t_pwg_block_ragged: int32 [ntiles][4] = {row b, first sample t0, valid samples W_b = lengths[b] * hop,
    0}, one entry per `tile`-sample tile that holds a valid sample, rows in order."""
    W = np.asarray(lengths, dtype=np.int64) * hop
    nt = (W + tile - 1) // tile
    b = np.repeat(np.arange(len(W)), nt)
    t0 = (np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)) * tile
    return np.stack([b, t0, W[b], np.zeros_like(b)], axis=1).astype(np.int32).reshape(-1, 4)


F16_MAX = 65504.0


def pwg_gate_perm(gate_channels: int = 128) -> np.ndarray:
    """Column order of the fused blocks' first product: column n' holds gate channel c = 32*(n'//64) + n'%32, its tanh half for
    (n'//32)%2 == 0, else its sigmoid half (channel c + gate_channels/2 of the convolution): a wave's two 32-column MFMA blocks
    then hold both pre-activations of the same 32 channels."""
    n = np.arange(gate_channels)
    return (n // 64) * 32 + n % 32 + (gate_channels // 2) * ((n // 32) % 2)


def _pack_pwg_block(conv_w, conv_b, aux_w, out_w, cast=torch.Tensor.contiguous):
    """Operands of the fused residual blocks from one block's parameters (CPU or device tensors; pure).

    conv_w (128, 64, 3) dilated conv, conv_b (128,), aux_w (128, 80[, 1]) conv1x1_aux, out_w (128, 64[, 1]) conv1x1_out ->
    w0 [272][128]: row k = tap*64 + in_channel for the taps at t-dil, t, t+dil, then 192 + aux channel (tap-major K
    order); column n' = pwg_gate_perm;  b0 fp32 [128] permuted the same way;  w1 [64][128] = conv1x1_out.weight^T.
    cast: what the two weight matrices pass through (the fp32 kernels: nothing)."""
    conv_w = torch.as_tensor(conv_w, dtype=torch.float32)
    G, R, taps = conv_w.shape
    aux_w = torch.as_tensor(aux_w, dtype=torch.float32).reshape(G, -1)
    out_w = torch.as_tensor(out_w, dtype=torch.float32).reshape(-1, G // 2)
    if (G, R, taps, aux_w.shape[1], out_w.shape[0]) != (128, 64, 3, 80, 128):
        raise ValueError("pwg block operands: the kernels are built for the v1 channel plan (64 / 128 / 64 / 80, kernel size 3)")
    perm = torch.as_tensor(pwg_gate_perm(G), device=conv_w.device)
    wk = conv_w.permute(0, 2, 1).reshape(G, taps * R)                       # [out][tap*64 + in]
    w0 = torch.cat([wk, aux_w.to(conv_w.device)], dim=1)[perm]               # [n'][272]
    b0 = torch.as_tensor(conv_b, dtype=torch.float32).to(conv_w.device)[perm].contiguous()
    return cast(w0.t()), b0, cast(out_w.to(conv_w.device).t())


def pack_pwg_block_f16(conv_w, conv_b, aux_w, out_w):
    """Operands of a3t_pwg_block_f16: _pack_pwg_block with w0h / w1h cast to fp16, round-to-nearest-even and saturated to
    +-65504."""
    return _pack_pwg_block(conv_w, conv_b, aux_w, out_w, lambda t: t.clamp(-F16_MAX, F16_MAX).to(torch.float16).contiguous())


class _WaveGeneratorHIP:
    """What the generators share: the device, the statistics of normalize_before and the preamble of inference."""

    def _setup(self, device, aux_channels, stats):
        self.dev, self.A = torch.device(device), int(aux_channels)
        self.stats = None
        if stats is not None:     # normalize_before of the pretrained wrapper (c - mean) / scale
            self.stats = (torch.as_tensor(stats["mean"], dtype=torch.float32, device=self.dev),
                          torch.as_tensor(stats["scale"], dtype=torch.float32, device=self.dev))

    def prepare(self, c, normalize_before, lengths, rates):
        """c (T_feats, aux) or (B, T_feats, aux) -> (c [B][Tf][A] fp32 on the device, single, lens, tiles).  lengths (host
        integers, one per row): lens = the device int32 [B] of them and tiles = {rate: pwg_tile_list(lengths, rate) on the device}
        for the samples-per-frame rates that fused kernels run at, else None and {}."""
        single = (c.dim() == 2)
        c = c.to(self.dev, torch.float32)
        if single:
            c = c[None]
        B, Tf, A = c.shape
        if A != self.A:
            raise ValueError(f"c has {A} channels, the generator {self.A}")
        if normalize_before and self.stats is not None:
            c = (c - self.stats[0]) / self.stats[1]
        if lengths is None:
            return c, single, None, {}
        if single:
            raise ValueError("lengths= goes with a (B, Tmax, aux) batch")
        lengths = [int(x) for x in lengths]
        if len(lengths) != B or any(n < 0 or n > Tf for n in lengths):
            raise ValueError(f"lengths {lengths} do not fit a batch of {B} rows of {Tf} frames")
        # one H2D copy: lens [B] | one tile list [ntiles][4] = {b, t0, W_b, 0} per rate (offsets kept 16-byte aligned)
        lists = [pwg_tile_list(lengths, r) for r in rates]
        offs = np.cumsum([(B + 3) // 4 * 4] + [tl.size for tl in lists]).tolist()
        host = np.zeros(offs[-1], dtype=np.int32)
        host[:B] = lengths
        for o, tl in zip(offs, lists):
            host[o:o + tl.size] = tl.reshape(-1)
        meta = torch.from_numpy(host).to(self.dev)
        return c, single, meta[:B], {r: meta[o:o + tl.size].view(len(tl), 4) for r, o, tl in zip(rates, offs, lists)}


class ParallelWaveGANGeneratorHIP(_WaveGeneratorHIP):
    """compute="f32" (default): exact fp32 products.  compute="f16": the residual blocks run on the 16-bit MFMA, one launch per
    block (pwg_fused_f16.hip): the conv input, the upsampled mel, the gate output and the block weights are rounded to fp16
    (nearest even, saturated), everything else stays fp32.  It needs the fused v1 channel plan."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", layers=30, stacks=3, residual_channels=64,
                 gate_channels=128, skip_channels=64, aux_channels=80, aux_context_window=2,
                 upsample_scales: Sequence[int] = (4, 5, 3, 5), stats: Optional[Dict[str, np.ndarray]] = None,
                 fused: Optional[bool] = None, compute: str = "f32"):
        if compute not in ("f32", "f16"):
            raise ValueError(f"compute must be 'f32' or 'f16', got {compute!r}")
        if compute == "f16":
            if (residual_channels, gate_channels, skip_channels, aux_channels) != (64, 128, 64, 80):
                raise ValueError("compute='f16' needs the v1 channel plan: 64 residual / 128 gate / 64 skip / 80 aux channels")
            if fused is not None and not fused:
                raise ValueError("compute='f16' is a mode of the fused residual blocks: fused=False cannot be combined with it")
            fused = True
        self.compute = compute
        self._setup(device, aux_channels, stats)
        self.layers, self.stacks = layers, stacks
        self.R, self.G, self.S = residual_channels, gate_channels, skip_channels
        self.ctx = aux_context_window
        self.scales = tuple(upsample_scales)
        self.upsample_factor = int(np.prod(self.scales))

        def t(k):
            return torch.as_tensor(np.asarray(state_dict[k]), dtype=torch.float32).to(self.dev)

        def conv(k):              # (out, in, taps) -> [out][tap][in]
            return t(k).permute(0, 2, 1).contiguous()

        self.w_first = t("first_conv.weight").reshape(self.R, 1).contiguous()
        self.b_first = t("first_conv.bias")
        self.w_in = conv("upsample_net.conv_in.weight")
        self.w_up = [t(f"upsample_net.upsample.up_layers.{2 * i + 1}.weight").reshape(-1).contiguous()
                     for i in range(len(self.scales))]
        # fused residual-block kernels (pwg_fused.hip) need the v1 channel plan: 64 residual / 128 gate / 64 skip / 80 aux
        if fused is None:
            fused = os.environ.get("A3T_PWG_FUSED", "1") != "0"
        self.fused = bool(fused) and (self.R, self.G, self.S, self.A) == (64, 128, 64, 80)
        self.blocks = []
        for l in range(layers):
            p = f"conv_layers.{l}."
            blk = dict(w=conv(p + "conv.weight"), b=t(p + "conv.bias"),
                       aux=t(p + "conv1x1_aux.weight").reshape(self.G, self.A).contiguous(),
                       out=t(p + "conv1x1_out.weight").reshape(self.R + self.S, self.G // 2).contiguous(),
                       bout=t(p + "conv1x1_out.bias"))
            if self.fused:      # wt0 [272][128] k-major in the gate permutation, wt1 [64][128]
                raw = (t(p + "conv.weight"), blk["b"], blk["aux"], blk["out"])
                blk["wt0"], blk["b0"], blk["wt1"] = _pack_pwg_block(*raw)
                if compute == "f16":
                    blk["w0h"], blk["b0h"], blk["w1h"] = pack_pwg_block_f16(*raw)
            self.blocks.append(blk)
        self.w_l1 = t("last_conv_layers.1.weight").reshape(self.S, self.S).contiguous()
        self.b_l1 = t("last_conv_layers.1.bias")
        self.w_l3 = t("last_conv_layers.3.weight").reshape(1, self.S).contiguous()
        self.b_l3 = t("last_conv_layers.3.bias")

    @torch.no_grad()
    def inference(self, c: torch.Tensor, z: Optional[torch.Tensor] = None, normalize_before: bool = False,
                  lengths: Optional[Sequence[int]] = None):
        """c (T_feats, aux) [or (B, T_feats, aux)], z (T_wav, 1) noise -> (T_wav, 1) [or (B, T_wav, 1)].

        lengths (host integers, one per row of a (B, Tmax, aux) batch): row b is computed exactly as if c[b, :L_b] (and
        z[b, :L_b * hop]) had been passed alone -- replicate padding, the smoothing and the dilated convolutions see the row's
        own end -- and the result (B, Tmax * hop, 1) is zero behind L_b * hop.  What the padding of c and z holds reaches no
        valid sample, and with the fused blocks the padding costs no time."""
        hop = self.upsample_factor
        c, single, lens, tiles = self.prepare(c, normalize_before, lengths, (hop,))
        tiles = tiles.get(hop)
        B, Tf, A = c.shape
        Tw = Tf * hop
        dev = self.dev
        if z is None:
            z = torch.randn(B, Tw, 1, device=dev)
        z = z.to(dev, torch.float32).reshape(B * Tw, 1).contiguous()
        # ---- ConvInUpsampleNetwork: replication pad, conv_in (k = 2*ctx+1, no bias), stretch+smooth per scale
        w = self.ctx
        Tp = Tf + 2 * w
        cp = torch.empty(B * Tp, A, device=dev)
        ops.replicate_pad(c.contiguous(), cp, w, lens)
        ci = torch.empty(B * Tp, A, device=dev)
        ops.conv_fwd(cp, self.w_in, ci, Tp, w, compute=F32)
        cu = ci.view(B, Tp, A)[:, w:w + Tf].contiguous()
        T, mul = Tf, 1
        for sc, wk in zip(self.scales, self.w_up):
            out = torch.empty(B, T * sc, A, device=dev)
            ops.pwg_upsample(cu, wk, out, sc, lens, mul)
            cu, T, mul = out, T * sc, mul * sc
        cu = cu.view(B * Tw, A)
        # ---- first conv (1 -> R), residual stack
        x = torch.empty(B * Tw, self.R, device=dev)
        ops.linear_fwd(z, self.w_first, x, bias=self.b_first, compute=F32)
        skips = torch.zeros(B * Tw, self.S, device=dev)
        if self.compute == "f16":
            cu16 = torch.empty(B * Tw, A, dtype=torch.float16, device=dev)
            ops.cast_f16_sat(cu, cu16)
            cu = cu16
        self._blocks(x, cu, skips, B, Tw, lens, tiles)
        ops.bias_act(skips, None, ACT_RELU, math.sqrt(1.0 / self.layers))
        h = torch.empty(B * Tw, self.S, device=dev)
        ops.linear_fwd(skips, self.w_l1, h, bias=self.b_l1, act=ACT_RELU, compute=F32)
        wav = torch.empty(B * Tw, 1, device=dev)
        ops.linear_fwd(h, self.w_l3, wav, bias=self.b_l3, compute=F32)
        if lens is not None:
            ops.zero_tail(wav, lens, hop, B, Tw)
        wav = wav.view(B, Tw, 1)
        return wav[0] if single else wav

    def _scratch(self, n):
        """The buffers of n = B * Tw samples that _blocks needs beside its arguments."""
        def e(C):
            return torch.empty(n, C, device=self.dev)
        if self.compute == "f16":
            return dict(x2=e(self.R))
        if self.fused:
            return dict(g=e(self.G // 2))
        return dict(y=e(self.G), ca=e(self.G), g=e(self.G // 2), o=e(self.R + self.S))

    def _blocks(self, x, cu, skips, B, Tw, lens=None, tiles=None, scratch=None):
        """The residual stack: skips is updated in place, and so is x except with compute="f16", which leaves it undefined.
        lens / tiles: rows of different length (lens [B] frames, tiles = pwg_tile_list of them, both on the device), else all
        rows are Tw samples long.  scratch: _scratch(B * Tw), for a caller that wants no allocation in here.

        compute="f16": cu is the fp16 cast (ops.cast_f16_sat) and x ping-pongs between two buffers (a block must not overwrite
        the x[t +- dil] that other tiles still read).  Layer by layer: the rows behind W_b of x are zeroed after every block,
        so that the convolution's taps beyond a row's end read zeros like those beyond Tmax; what the tail of y / g / o / skips
        holds never reaches a valid row."""
        s = scratch if scratch is not None else self._scratch(B * Tw)
        hop, lps = self.upsample_factor, self.layers // self.stacks
        if not self.fused and lens is not None:
            ops.zero_tail(x, lens, hop, B, Tw)
        x2 = s.get("x2")
        for l, blk in enumerate(self.blocks):
            dil = 2 ** (l % lps)
            if self.compute == "f16":
                ops.pwg_block_f16(x, x2, cu, blk["w0h"], blk["b0h"], blk["w1h"], blk["bout"], skips, tiles, B, Tw, dil)
                x, x2 = x2, x
            elif self.fused:
                ops.pwg_block(x, cu, blk["wt0"], blk["b0"], blk["wt1"], blk["bout"], s["g"], skips, B, Tw, dil, tiles)
            else:
                ops.conv_fwd(x, blk["w"], s["y"], Tw, 1, dil, bias=blk["b"], compute=F32)
                ops.linear_fwd(cu, blk["aux"], s["ca"], compute=F32)
                ops.pwg_gate(s["y"], s["ca"], s["g"])
                ops.linear_fwd(s["g"], blk["out"], s["o"], bias=blk["bout"], compute=F32)
                ops.pwg_res_skip(s["o"], x, skips)
                if lens is not None:
                    ops.zero_tail(x, lens, hop, B, Tw)

    @property
    def margin_frames(self) -> int:
        """pwg_margin_frames of this generator's configuration (kernel size 3: the only one the class builds)."""
        return pwg_margin_frames(self.layers, self.stacks, 3, self.scales, self.ctx)

    __call__ = inference


# ---------------------------------------------------------------------------------------------------- HiFi-GAN generator
def hifigan_margin_frames(upsample_scales: Sequence[int] = (5, 5, 4, 3), resblock_kernel_sizes: Sequence[int] = (3, 7, 11),
                          resblock_dilations=((1, 3, 5),) * 3, kernel_size: int = 7, use_additional_convs: bool = True) -> int:
    """pwg_margin_frames for the HiFi-GAN generator.  Walked from the output back to the mel: the output convolution reaches
    (K-1)/2 samples; the residual blocks of stage i max_j sum_d (k_j-1)/2 * (d + 1) samples of stage i (+ 1: the additional
    convolution of dilation 1; without it sum_d (k_j-1)/2 * d); a transposed convolution of scale s turns a reach of n output
    samples into ceil(n / s) + 1 input samples (output q*s + r reads inputs q-1 .. q+1); the input convolution adds (K-1)/2
    frames.  20 for the 24 kHz v1 plan (5, 5, 4, 3) x (3, 7, 11) x (1, 3, 5), K = 7 (a probe of a model of that plan: 19
    reproduces the span, 18 does not: the ceil of each stage is what the formula gives away)."""
    extra = 1 if use_additional_convs else 0
    reach = max(sum((int(k) - 1) // 2 * (int(d) + extra) for d in dils)
                for k, dils in zip(resblock_kernel_sizes, resblock_dilations))
    n = (int(kernel_size) - 1) // 2
    for s in reversed([int(s) for s in upsample_scales]):
        n = -(-(n + reach) // s) + 1
    return n + (int(kernel_size) - 1) // 2


def fold_weight_norm(state_dict, prefix: str) -> torch.Tensor:
    """`prefix`.weight of a state dict as fp32, from the plain tensor or from weight_g / weight_v (torch.nn.utils.weight_norm
    with its default dim = 0: w = g * v / ||v||, the norm over all dims but the first -- for a ConvTranspose1d [Cin][Cout][k]
    that is dims 1, 2), folded in fp64."""
    if prefix + ".weight" in state_dict:
        return torch.as_tensor(np.asarray(state_dict[prefix + ".weight"]), dtype=torch.float32)
    g = torch.as_tensor(np.asarray(state_dict[prefix + ".weight_g"]), dtype=torch.float64)
    v = torch.as_tensor(np.asarray(state_dict[prefix + ".weight_v"]), dtype=torch.float64)
    norm = v.flatten(1).norm(dim=1).reshape(-1, *([1] * (v.dim() - 1)))
    return (g * v / norm).to(torch.float32)


def pack_hifigan_upsample(w: torch.Tensor, scale: int) -> torch.Tensor:
    """ConvTranspose1d(k = 2s, stride s, padding = ceil(s/2), output_padding = s % 2) as a 3-tap stride-1 convolution with
    N = s * Cout output columns (pure; any dtype).  w [Cin][Cout][2s] -> Wk [s*Cout][3][Cin] for ops.conv_fwd(pad=1): output
    sample q*s + r, channel co (column r*Cout + co) reads input q + t - 1 through w[:, co, (1 - t)*s + r + ceil(s/2)], zero where
    that index leaves [0, 2s).  The [B*T][s*Cout] result is the [B*T*s][Cout] tensor."""
    s = int(scale)
    Cin, Cout, k = w.shape
    if k != 2 * s:
        raise ValueError(f"pack_hifigan_upsample: kernel size {k} is not 2 * scale {s}")
    p = (s + 1) // 2
    Wk = torch.zeros(s, Cout, 3, Cin, dtype=w.dtype, device=w.device)
    for t in range(3):
        for r in range(s):
            i = (1 - t) * s + r + p
            if 0 <= i < k:
                Wk[r, :, t, :] = w[:, :, i].t()
    return Wk.reshape(s * Cout, 3, Cin).contiguous()


def pack_hifigan_conv(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [Cout][Cin][k] -> the k-major operand of a3t_hfg_conv [k*Cin][Cout] (row = tap*Cin + in channel)."""
    Cout, Cin, k = w.shape
    return w.permute(2, 1, 0).reshape(k * Cin, Cout).contiguous()


def pack_hifigan_conv_f16(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [Cout][Cin][k] fp32 (Cout = Cin = C, a multiple of 32) -> the fp16 operand of a3t_hfg_conv_f16 (pure torch, any
    device): the MFMA's A fragments in the order the kernel streams them, P [k*C/16][C/32][64][8] with

        P[ks][mt][l][j] = fp16(w[32*mt + (l & 31)][16*(ks % (C/16)) + 8*(l >> 5) + j][ks // (C/16)])

    (k-step ks = tap-major, 16 input channels each; M-tile mt = 32 output channels; lane l; element j), rounded to nearest even and
    saturated to +-65504."""
    Cout, Cin, k = w.shape
    if Cout != Cin or Cout % 32:
        raise ValueError(f"pack_hifigan_conv_f16: weight {tuple(w.shape)} is not [C][C][k] with C a multiple of 32")
    C = Cout
    t = w.to(torch.float32).clamp(-65504.0, 65504.0).to(torch.float16)
    t = t.permute(2, 1, 0).reshape(k, C // 16, 2, 8, C // 32, 32)      # [tap][ci / 16][l >> 5][j][mt][l & 31]
    return t.permute(0, 1, 4, 2, 5, 3).reshape(k * (C // 16), C // 32, 64, 8).contiguous()


F16_WIDTHS = (32, 64, 128, 256)      # the stage widths whose residual blocks compute="f16" moves to a3t_hfg_conv_f16


class HiFiGANGeneratorHIP(_WaveGeneratorHIP):
    """HiFi-GAN generator inference (espnet2/gan_tts/hifigan/hifigan.py:25-221, state-dict compatible with the
    parallel_wavegan zoo's HiFiGANGenerator), channels-last fp32 [B*T][C] on the device.

    fused=False: layer by layer -- a3t_leaky_relu in front of every convolution, every convolution (the transposed ones as
    3-tap convolutions, pack_hifigan_upsample) on the exact-fp32 GEMM.  fused=True: the residual blocks of the stages with 32 or
    64 channels run on a3t_hfg_conv (LeakyReLU, bias, residual and the MRF mean inside the launch) and the output convolution
    on a3t_hfg_out; stages of another width run layer by layer.  fused=True is the default because it is the faster path on the v1
    plan (profiles/hifigan_latency.txt: 46 ms against 83 ms for 8 x 1000 frames).

    compute="f16" (opt-in; needs fused=True): the residual blocks of every stage with C in F16_WIDTHS and kernels <= 11 run on
    a3t_hfg_conv_f16 -- in each of their convolutions leaky(x) is computed in fp32 and rounded to fp16 (nearest even, saturated
    to +-65504), the weight is rounded to fp16 once here, after the fp64 weight-norm fold, products accumulate in fp32.  Biases,
    residuals, the MRF mean and every tensor in memory stay fp32, and so do the input, transposed and output convolutions and
    the stages of another width.  compute="f32" (the default) is the exact-fp32 path, bit for bit what it was."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", in_channels=80, channels=512, kernel_size=7,
                 upsample_scales: Sequence[int] = (5, 5, 4, 3), upsample_kernel_sizes: Sequence[int] = (10, 10, 8, 6),
                 resblock_kernel_sizes: Sequence[int] = (3, 7, 11), resblock_dilations=((1, 3, 5),) * 3,
                 use_additional_convs=True, bias=True, negative_slope=0.1, stats: Optional[Dict[str, np.ndarray]] = None,
                 fused=True, compute="f32"):
        if compute not in ("f32", "f16"):
            raise ValueError(f"compute must be 'f32' or 'f16', got {compute!r}")
        if compute == "f16" and not fused:
            raise ValueError("compute='f16' is a mode of the fused kernels: it needs fused=True")
        self.compute = compute
        self.scales = tuple(int(s) for s in upsample_scales)
        self.rk = tuple(int(k) for k in resblock_kernel_sizes)
        self.rd = tuple(tuple(int(d) for d in ds) for ds in resblock_dilations)
        if kernel_size % 2 == 0:
            raise ValueError(f"kernel_size {kernel_size} must be odd")
        if any(k % 2 == 0 for k in self.rk):
            raise ValueError(f"resblock_kernel_sizes {list(self.rk)} must be odd")
        if len(upsample_kernel_sizes) != len(self.scales) or any(int(k) != 2 * s for k, s in zip(upsample_kernel_sizes, self.scales)):
            raise ValueError(f"upsample_kernel_sizes {list(upsample_kernel_sizes)} must be twice upsample_scales {list(self.scales)}")
        if len(self.rk) != len(self.rd):
            raise ValueError("resblock_dilations must have one list per entry of resblock_kernel_sizes")
        if channels % (2 ** len(self.scales)):
            raise ValueError(f"channels {channels} must be divisible by 2^{len(self.scales)}")
        self._setup(device, in_channels, stats)
        self.C0, self.K = int(channels), int(kernel_size)
        self.add, self.slope = bool(use_additional_convs), float(negative_slope)
        self.upsample_factor = int(np.prod(self.scales))

        def w(p):
            return fold_weight_norm(state_dict, p)

        def b(p, n, rep=1):
            if not bias and p + ".bias" not in state_dict:
                return None
            v = torch.as_tensor(np.asarray(state_dict[p + ".bias"]), dtype=torch.float32)
            if v.numel() != n:
                raise ValueError(f"{p}.bias has {v.numel()} entries, expected {n}")
            return v.repeat(rep).contiguous().to(self.dev)

        def conv(t):              # (out, in, taps) -> [out][tap][in]
            return t.permute(0, 2, 1).contiguous().to(self.dev)

        self.w_in, self.b_in = conv(w("input_conv")), torch.as_tensor(np.asarray(state_dict["input_conv.bias"]),
                                                                      dtype=torch.float32).to(self.dev)
        if tuple(self.w_in.shape) != (self.C0, self.K, self.A):
            raise ValueError(f"input_conv.weight {tuple(self.w_in.shape)} does not fit channels / kernel_size / in_channels")
        self.stages = []
        for i, s in enumerate(self.scales):
            C = self.C0 >> (i + 1)
            f16 = compute == "f16" and C in F16_WIDTHS and max(self.rk) <= 11
            st = dict(C=C, s=s, f16=f16, w_up=pack_hifigan_upsample(w(f"upsamples.{i}.1"), s).to(self.dev),
                      b_up=torch.as_tensor(np.asarray(state_dict[f"upsamples.{i}.1.bias"]), dtype=torch.float32).repeat(s).to(self.dev),
                      fused=f16 or (bool(fused) and C in (32, 64) and max(self.rk) <= 11), blocks=[])
            for j, (k, dils) in enumerate(zip(self.rk, self.rd)):
                units = []
                for d in range(len(dils)):
                    p = f"blocks.{i * len(self.rk) + j}."
                    names = [p + f"convs1.{d}.1"] + ([p + f"convs2.{d}.1"] if self.add else [])
                    ws = [w(n) for n in names]
                    units.append(dict(dil=dils[d], b=[b(n, C) for n in names],
                                      w=[(pack_hifigan_conv_f16(t).to(self.dev) if f16 else
                                          pack_hifigan_conv(t).to(self.dev) if st["fused"] else conv(t)) for t in ws]))
                st["blocks"].append(dict(k=k, units=units))
            self.stages.append(st)
        Cl = self.C0 >> len(self.scales)
        w_out = w("output_conv.1")
        if tuple(w_out.shape) != (1, Cl, self.K):
            raise NotImplementedError(f"out_channels: output_conv.1.weight {tuple(w_out.shape)} is not (1, {Cl}, {self.K})")
        self.w_out = conv(w_out)                                      # [1][K][Cl]
        self.b_out = torch.as_tensor(np.asarray(state_dict["output_conv.1.bias"]), dtype=torch.float32).to(self.dev)
        self.fused_out = bool(fused) and Cl <= 64 and Cl % 4 == 0 and self.K <= 11
        self.fused = any(st["fused"] for st in self.stages)

    @classmethod
    def from_config(cls, state_dict, generator_params: Dict, generator_type: str = "HiFiGANGenerator", **kw):
        """From the `generator_params` (and `generator_type`) of a parallel_wavegan config.yml and the checkpoint's
        model["generator"] state dict.  kw: device, stats, fused, compute."""
        if generator_type != "HiFiGANGenerator":
            raise NotImplementedError(f"generator_type {generator_type!r}: only HiFiGANGenerator is built here")
        p = dict(generator_params)
        if int(p.pop("out_channels", 1)) != 1:
            raise NotImplementedError("out_channels != 1 is not supported (no multi-band / PQMF synthesis)")
        if int(p.pop("global_channels", -1)) > 0:
            raise NotImplementedError("global_channels > 0 (global conditioning) is not supported")
        act = p.pop("nonlinear_activation", "LeakyReLU")
        if act != "LeakyReLU":
            raise NotImplementedError(f"nonlinear_activation {act!r}: only LeakyReLU is built into the kernels")
        if p.pop("use_causal_conv", False):
            raise NotImplementedError("use_causal_conv is not supported")
        ap = dict(p.pop("nonlinear_activation_params", None) or {"negative_slope": 0.1})
        p.pop("use_weight_norm", None)      # the state dict says which form it holds
        if "upsample_kernal_sizes" in p:    # (the zoo's older configs spell it so)
            p["upsample_kernel_sizes"] = p.pop("upsample_kernal_sizes")
        known = ("in_channels", "channels", "kernel_size", "upsample_scales", "upsample_kernel_sizes", "resblock_kernel_sizes",
                 "resblock_dilations", "use_additional_convs", "bias")
        unknown = sorted(set(p) - set(known))
        if unknown:
            raise NotImplementedError(f"generator_params {unknown} are not understood")
        return cls(state_dict, negative_slope=float(ap.get("negative_slope", 0.01)), **p, **kw)

    @property
    def margin_frames(self) -> int:
        return hifigan_margin_frames(self.scales, self.rk, self.rd, self.K, self.add)

    def _lrelu(self, x, slope=None):
        y = torch.empty_like(x)
        ops.leaky_relu(x, y, self.slope if slope is None else slope)
        return y

    @torch.no_grad()
    def inference(self, c: torch.Tensor, z: Optional[torch.Tensor] = None, normalize_before: bool = False,
                  lengths: Optional[Sequence[int]] = None):
        """c (T_feats, aux) [or (B, T_feats, aux)] -> (T_wav, 1) [or (B, T_wav, 1)]; z must be None (HiFi-GAN has no noise input).

        lengths (host integers, one per row of a (B, Tmax, aux) batch): row b is computed exactly as if c[b, :L_b] had been
        passed alone -- every convolution reads zeros behind the row's end at its own rate and stores zeros there -- and the
        result (B, Tmax * hop, 1) is zero behind L_b * hop.  What the padding of c holds reaches no valid sample."""
        if z is not None:
            raise ValueError("HiFiGANGeneratorHIP.inference: z must be None, the HiFi-GAN generator has no noise input")
        rates, r = [], 1      # the rates of the fused kernels
        for st in self.stages:
            r *= st["s"]
            if st["fused"]:
                rates.append(r)
        if self.fused_out and r not in rates:
            rates.append(r)
        c, single, lens, tiles = self.prepare(c, normalize_before, lengths, rates)
        B, Tf, A = c.shape
        dev = self.dev

        def tail(x, rate, T):
            if lens is not None:
                ops.zero_tail(x, lens, rate, B, T)

        c = c.contiguous()
        if lens is not None:      # (a copy: c may be the caller's tensor)
            c = c.clone()
            tail(c, 1, Tf)
        x = torch.empty(B * Tf, self.C0, device=dev)
        ops.conv_fwd(c.view(B * Tf, A), self.w_in, x, Tf, (self.K - 1) // 2, bias=self.b_in, compute=F32)
        tail(x, 1, Tf)
        T, rate = Tf, 1
        for st in self.stages:
            C, s = st["C"], st["s"]
            up = torch.empty(B * T, s * C, device=dev)
            ops.conv_fwd(self._lrelu(x), st["w_up"], up, T, 1, bias=st["b_up"], compute=F32)
            T, rate = T * s, rate * s
            up = up.view(B * T, C)
            tail(up, rate, T)
            run = self._stage_fused if st["fused"] else self._stage_layers
            x = run(st, up, B, T, rate, lens, tiles.get(rate))
        wav = torch.empty(B * T, 1, device=dev)
        if self.fused_out:
            if lens is not None:      # the kernel writes no sample behind a row's end
                wav.zero_()
            ops.hfg_out(x, self.w_out.view(self.K, -1), self.b_out, wav, B, T, 0.01, tiles.get(rate))
        else:
            ops.conv_fwd(self._lrelu(x, 0.01), self.w_out, wav, T, (self.K - 1) // 2, bias=self.b_out, act=ACT_TANH, compute=F32)
            tail(wav, rate, T)
        wav = wav.view(B, T, 1)
        return wav[0] if single else wav

    def _stage_layers(self, st, up, B, T, rate, lens, tiles):
        """The residual blocks of one stage and their mean, layer by layer: (sum_j block_j(up)) / num_blocks, the division
        deliberately as one multiplication by fp32(1 / num_blocks) (a3t_scale): at most one ulp from the reference's quotient."""
        bufs = [torch.empty_like(up) for _ in range(3)]
        cs = torch.empty_like(up)
        for j, blk in enumerate(st["blocks"]):
            pad, x = (blk["k"] - 1) // 2, up
            for u, unit in enumerate(blk["units"]):
                xn, xt = bufs[u % 2], bufs[2]
                if self.add:
                    ops.conv_fwd(self._lrelu(x), unit["w"][0], xt, T, pad, unit["dil"], bias=unit["b"][0], compute=F32)
                    if lens is not None:
                        ops.zero_tail(xt, lens, rate, B, T)
                    ops.conv_fwd(self._lrelu(xt), unit["w"][1], xn, T, pad, 1, bias=unit["b"][1], R=x, compute=F32)
                else:
                    ops.conv_fwd(self._lrelu(x), unit["w"][0], xn, T, pad, unit["dil"], bias=unit["b"][0], R=x, compute=F32)
                if lens is not None:
                    ops.zero_tail(xn, lens, rate, B, T)
                x = xn
            if j == 0:
                cs.copy_(x)
            else:
                ops.axpy(x, cs, 1.0)
        ops.scale(cs, cs, 1.0 / len(st["blocks"]))
        return cs

    def _stage_fused(self, st, up, B, T, rate, lens, tiles):
        """The same on a3t_hfg_conv (a3t_hfg_conv_f16 for a stage of compute="f16"): the last convolution of block j leaves
        alpha * block_j in the mean's buffer (alpha = 1 / num_blocks), so block outputs are never stored.  Rows behind a row's end
        are not written by the kernel: the mean's buffer starts as zeros there for the (unragged) convolution that reads it next."""
        bufs = [torch.empty_like(up) for _ in range(3)]
        cs = torch.zeros_like(up) if lens is not None else torch.empty_like(up)
        alpha = 1.0 / len(st["blocks"])
        conv = ops.hfg_conv_f16 if st["f16"] else ops.hfg_conv
        for j, blk in enumerate(st["blocks"]):
            x = up
            for u, unit in enumerate(blk["units"]):
                xn, xt = bufs[u % 2], bufs[2]
                if u == len(blk["units"]) - 1:
                    out = dict(y=None, acc=cs, alpha=alpha, acc_add=j > 0)
                else:
                    out = dict(y=xn)
                src, dil = x, unit["dil"]
                if self.add:
                    conv(x, unit["w"][0], unit["b"][0], xt, B, T, dil, self.slope, tiles=tiles)
                    src, dil = xt, 1
                conv(src, unit["w"][-1], unit["b"][-1], out.pop("y"), B, T, dil, self.slope, R=x, tiles=tiles, **out)
                x = xn
        return cs

    __call__ = inference
