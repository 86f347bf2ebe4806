"""ParallelWaveGAN generator inference on the GPU (mel -> waveform).

Mirror of the vocoder the reference calls in ``sedit_inference.py:77,339-348`` through
``ParallelWaveGANPretrainedVocoder`` (espnet2/tts/utils/parallel_wavegan_pretrained_vocoder.py:49-63);
the network restated is the vendored twin ``ParallelWaveGANGenerator``
(espnet2/gan_tts/parallel_wavegan/parallel_wavegan.py:136-229, wavenet/residual_block.py:114-169,
parallel_wavegan/upsample.py:22-189), weight-norm removed.  Layout is channels-last [T][C] so every
Conv1d (dilated k=3, 1x1) is the shared implicit-im2col MFMA GEMM; the gated activation, residual /
skip update and nearest-neighbour upsampling+smoothing are element-wise HIP kernels.
"""
import math
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import ACT_RELU, F32


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


def pack_pwg_block_f16(conv_w, conv_b, aux_w, out_w):
    """Operands of a3t_pwg_block_f16 from one residual block's parameters (CPU or device tensors; pure).

    conv_w (128, 64, 3) dilated conv, conv_b (128,), aux_w (128, 80[, 1]) conv1x1_aux, out_w (128, 64[, 1]) conv1x1_out ->
    w0h fp16 [272][128]: row k = tap*64 + in_channel for the taps at t-dil, t, t+dil, then 192 + aux channel (tap-major K
    order); column n' = pwg_gate_perm;  b0 fp32 [128] permuted the same way;  w1h fp16 [64][128] = conv1x1_out.weight^T.
    The cast is round-to-nearest-even and saturates to +-65504."""
    conv_w = torch.as_tensor(conv_w, dtype=torch.float32)
    G, R, taps = conv_w.shape
    aux_w = torch.as_tensor(aux_w, dtype=torch.float32).reshape(G, -1)
    out_w = torch.as_tensor(out_w, dtype=torch.float32).reshape(-1, G // 2)
    if (G, R, taps, aux_w.shape[1], out_w.shape[0]) != (128, 64, 3, 80, 128):
        raise ValueError("pack_pwg_block_f16: the kernel is built for the v1 channel plan (64 / 128 / 64 / 80, kernel size 3)")
    perm = torch.as_tensor(pwg_gate_perm(G), device=conv_w.device)
    wk = conv_w.permute(0, 2, 1).reshape(G, taps * R)                       # [out][tap*64 + in]
    w0 = torch.cat([wk, aux_w.to(conv_w.device)], dim=1)[perm]               # [n'][272]

    def h(t):
        return t.clamp(-F16_MAX, F16_MAX).to(torch.float16).contiguous()

    b0 = torch.as_tensor(conv_b, dtype=torch.float32).to(conv_w.device)[perm].contiguous()
    return h(w0.t()), b0, h(out_w.to(conv_w.device).t())


class ParallelWaveGANGeneratorHIP:
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
        self.dev = torch.device(device)
        self.layers, self.stacks = layers, stacks
        self.R, self.G, self.S, self.A = residual_channels, gate_channels, skip_channels, aux_channels
        self.ctx = aux_context_window
        self.scales = tuple(upsample_scales)
        self.upsample_factor = int(np.prod(self.scales))
        self.stats = None
        if stats is not None:     # normalize_before of the pretrained wrapper (c - mean) / scale
            self.stats = (torch.as_tensor(stats["mean"], dtype=torch.float32, device=self.dev),
                          torch.as_tensor(stats["scale"], dtype=torch.float32, device=self.dev))

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
        # stage-0 output column n' holds gate channel c = 32*(n'//64) + n'%32, tanh half for (n'//32)%2 == 0 else sigmoid
        npr = np.arange(128)
        perm = torch.as_tensor((npr // 64) * 32 + npr % 32 + 64 * ((npr // 32) % 2), device=self.dev)
        self.blocks = []
        for l in range(layers):
            p = f"conv_layers.{l}."
            blk = dict(w=conv(p + "conv.weight"), b=t(p + "conv.bias"),
                       aux=t(p + "conv1x1_aux.weight").reshape(self.G, self.A).contiguous(),
                       out=t(p + "conv1x1_out.weight").reshape(self.R + self.S, self.G // 2).contiguous(),
                       bout=t(p + "conv1x1_out.bias"))
            if self.fused:
                wk = blk["w"].reshape(self.G, 3 * self.R)                       # [out][tap*64 + in]
                w0 = torch.cat([wk, blk["aux"]], dim=1)[perm]                   # [n'][272]
                blk["wt0"] = w0.t().contiguous()                                # [272][128] k-major
                blk["b0"] = blk["b"][perm].contiguous()
                blk["wt1"] = blk["out"].t().contiguous()                        # [64][128]
            if compute == "f16":
                blk["w0h"], blk["b0h"], blk["w1h"] = pack_pwg_block_f16(t(p + "conv.weight"), blk["b"], blk["aux"], blk["out"])
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
        single = (c.dim() == 2)
        c = c.to(self.dev, torch.float32)
        if single:
            c = c[None]
        B, Tf, A = c.shape
        if normalize_before and self.stats is not None:
            c = (c - self.stats[0]) / self.stats[1]
        if lengths is not None and single:
            raise ValueError("lengths= goes with a (B, Tmax, aux) batch")
        hop = self.upsample_factor
        Tw = Tf * hop
        dev = self.dev
        lens = tiles = None
        if lengths is not None:
            lengths = [int(x) for x in lengths]
            if len(lengths) != B or any(n < 0 or n > Tf for n in lengths):
                raise ValueError(f"lengths {lengths} do not fit a batch of {B} rows of {Tf} frames")
            # one H2D copy: lens [B] | tile list [ntiles][4] = {b, t0, W_b, 0} for the fused blocks (offset kept 16-byte aligned)
            tl = pwg_tile_list(lengths, hop)
            off = (B + 3) // 4 * 4
            host = np.zeros(off + tl.size, dtype=np.int32)
            host[:B] = lengths
            host[off:] = tl.reshape(-1)
            meta = torch.from_numpy(host).to(dev)
            lens, tiles = meta[:B], meta[off:].view(len(tl), 4)
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
