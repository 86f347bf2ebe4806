"""Neural vocoders on the GPU (mel -> waveform): the four generator families of the parallel_wavegan model zoo.

ParallelWaveGANGeneratorHIP mirrors the vocoder the reference calls in ``sedit_inference.py:77,339-348`` through
``ParallelWaveGANPretrainedVocoder`` (espnet2/tts/utils/parallel_wavegan_pretrained_vocoder.py:49-63);
the network restated is the vendored twin ``ParallelWaveGANGenerator``
(espnet2/gan_tts/parallel_wavegan/parallel_wavegan.py:136-229, wavenet/residual_block.py:114-169,
parallel_wavegan/upsample.py:22-189), weight-norm removed.  Layout is channels-last [T][C] so every
Conv1d (dilated k=3, 1x1) is the shared implicit-im2col MFMA GEMM; the gated activation, residual /
skip update and nearest-neighbour upsampling+smoothing are element-wise HIP kernels.

HiFiGANGeneratorHIP, MelGANGeneratorHIP (MelGAN and multi-band MelGAN) and StyleMelGANGeneratorHIP have the same inference
interface.  _WaveGeneratorHIP holds what the four share: the weight loader, the preamble of inference and the stage helpers;
_config_params is the one reading of a checkpoint's generator_params.  generator_from_config picks the class from a checkpoint's
config (StyleMelGANGeneratorHIP is built through its own from_config; generator_from_config does not dispatch to it yet).
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


def span_windows(spans: Sequence[Sequence[int]], T: int, margin: int):
    """span_window per span of [[n0, n1], ...] (left to right), windows that touch or overlap merged into one: the frame
    windows to vocode so that every span's samples come out as in a run over the whole utterance."""
    wins = []
    for n0, n1 in spans:
        w0, w1 = span_window(n0, n1, T, margin)
        if wins and w0 <= wins[-1][1]:
            wins[-1] = (min(wins[-1][0], w0), max(wins[-1][1], w1))
        else:
            wins.append((w0, w1))
    return wins


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


def _check_compute(compute: str) -> str:
    if compute not in ("f32", "f16"):
        raise ValueError(f"compute must be 'f32' or 'f16', got {compute!r}")
    return compute


def _tap_major(t: torch.Tensor, device) -> torch.Tensor:
    """Conv1d weight (out, in, taps) -> the operand [out][tap][in] of ops.conv_fwd, on the device."""
    return t.permute(0, 2, 1).contiguous().to(device)


def _config_params(p: Dict, known: Sequence[str], fixed: Dict) -> Dict:
    """What is left of p, a copy of a config's generator_params, for a constructor that takes the `known` keys.  fixed
    {field: (the only value built here, the refusal's text)}: such a field is dropped, or refused by name
    (NotImplementedError; {!r} in the text is the value asked for), and so is every key that is not known.  use_weight_norm is
    dropped: the state dict says which form it holds."""
    p.pop("use_weight_norm", None)
    for k, (v, msg) in fixed.items():
        if k in p and p[k] != v:
            raise NotImplementedError(msg.format(p[k]))
        p.pop(k, None)
    unknown = sorted(set(p) - set(known))
    if unknown:
        raise NotImplementedError(f"generator_params {unknown} are not understood")
    return p


_LRELU_ONLY = ("LeakyReLU", "nonlinear_activation {!r}: only LeakyReLU is built into the kernels")
_NOT_CAUSAL = (False, "use_causal_conv is not supported")


class _WaveGeneratorHIP:
    """What the generators share: the device, the statistics of normalize_before, the weight loader (_w, _b over the state
    dict that _setup is given), the preamble of inference (prepare = _check_input + _pack_meta) and the stage helpers."""

    def _setup(self, device, aux_channels, stats, state_dict, bias=True):
        self.dev, self.A = torch.device(device), int(aux_channels)
        self._sd, self._bias = state_dict, bool(bias)      # (for _w / _b; __init__ drops the state dict when it has loaded)
        self.stats = None
        if stats is not None:     # normalize_before of the pretrained wrapper (c - mean) / scale
            self.stats = (torch.as_tensor(stats["mean"], dtype=torch.float32, device=self.dev),
                          torch.as_tensor(stats["scale"], dtype=torch.float32, device=self.dev))

    def _w(self, p):
        """`p`.weight as fp32 on the host, weight norm folded."""
        return fold_weight_norm(self._sd, p)

    def _b(self, p, n, rep=1):
        """`p`.bias (n entries, checked) repeated rep times, on the device; None where a bias=False plan has none."""
        if not self._bias and p + ".bias" not in self._sd:
            return None
        v = torch.as_tensor(np.asarray(self._sd[p + ".bias"]), dtype=torch.float32)
        if v.numel() != n:
            raise ValueError(f"{p}.bias has {v.numel()} entries, expected {n}")
        return v.repeat(rep).contiguous().to(self.dev)

    def _check_input(self, c, normalize_before, lengths):
        """c (T_feats, aux) or (B, T_feats, aux) -> (c [B][Tf][A] fp32 on the device, normalised; single; lengths as a list of
        B integers in [0, Tf], or None)."""
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
            return c, single, None
        if single:
            raise ValueError("lengths= goes with a (B, Tmax, aux) batch")
        lengths = [int(x) for x in lengths]
        if len(lengths) != B or any(n < 0 or n > Tf for n in lengths):
            raise ValueError(f"lengths {lengths} do not fit a batch of {B} rows of {Tf} frames")
        return c, single, lengths

    def _pack_meta(self, vectors, tile_lengths, rates):
        """One H2D copy: the per-row int32 vectors [B] | one tile list [ntiles][4] = {b, t0, W_b, 0} per rate, pwg_tile_list(
        tile_lengths, rate) (offsets kept 16-byte aligned) -> (the vectors on the device, {rate: its tile list on the device})."""
        B = len(tile_lengths)
        Bp = (B + 3) // 4 * 4
        lists = [pwg_tile_list(tile_lengths, r) for r in rates]
        offs = np.cumsum([len(vectors) * Bp] + [tl.size for tl in lists]).tolist()
        host = np.zeros(offs[-1], dtype=np.int32)
        for i, v in enumerate(vectors):
            host[i * Bp:i * Bp + B] = v
        for o, tl in zip(offs, lists):
            host[o:o + tl.size] = tl.reshape(-1)
        meta = torch.from_numpy(host).to(self.dev)
        return ([meta[i * Bp:i * Bp + B] for i in range(len(vectors))],
                {r: meta[o:o + tl.size].view(len(tl), 4) for r, o, tl in zip(rates, offs, lists)})

    def prepare(self, c, normalize_before, lengths, rates):
        """c (T_feats, aux) or (B, T_feats, aux) -> (c [B][Tf][A] fp32 on the device, single, lens, tiles).  lengths (host
        integers, one per row): lens = the device int32 [B] of them and tiles = {rate: pwg_tile_list(lengths, rate) on the device}
        for the samples-per-frame rates that fused kernels run at, else None and {}."""
        c, single, lengths = self._check_input(c, normalize_before, lengths)
        if lengths is None:
            return c, single, None, {}
        (lens,), tiles = self._pack_meta([lengths], lengths, rates)
        return c, single, lens, tiles

    # ---- stage helpers: lens None = all rows full length, and nothing is zeroed
    def _lrelu(self, x, slope=None):
        y = torch.empty_like(x)
        ops.leaky_relu(x, y, self.slope if slope is None else slope)
        return y

    @staticmethod
    def _zero_tail(x, lens, rate, B, T):
        if lens is not None:
            ops.zero_tail(x, lens, rate, B, T)

    def _ragged_copy(self, c, lens):
        """c [B][Tf][A] contiguous; of a ragged batch a copy (c may be the caller's tensor) that is zero behind each row's end."""
        c = c.contiguous()
        if lens is not None:
            c = c.clone()
            ops.zero_tail(c, lens, 1, c.shape[0], c.shape[1])
        return c

    def _tiled_rates(self, out=()):
        """The samples-per-frame rates of the tiled kernels: those of the fused stages, then the last stage's times each of `out`."""
        rates, r = [], 1
        for st in self.stages:
            r *= st["s"]
            if st["fused"]:
                rates.append(r)
        return rates + [r * m for m in out if r * m not in rates]

    def _upsample(self, x, w, b, B, T, s, C, lens, rate, slope, after=False):
        """One transposed convolution of scale s as a 3-tap convolution (w, b: pack_hifigan_upsample and the bias repeated s times):
        x [B*T][Cin] at `rate` -> [B*T*s][C], zero behind lens * rate * s.  The LeakyReLU runs in front of it, or with `after`
        behind it, in place."""
        up = torch.empty(B * T, s * C, device=self.dev)
        ops.conv_fwd(x if after else self._lrelu(x, slope), w, up, T, 1, bias=b, compute=F32)
        up = up.view(B * T * s, C)
        if after:
            ops.leaky_relu(up, up, slope)
        self._zero_tail(up, lens, rate * s, B, T * s)
        return up


_PWG_KNOWN = ("layers", "stacks", "residual_channels", "gate_channels", "skip_channels", "aux_channels", "aux_context_window",
              "upsample_params")
_PWG_FIXED = dict(in_channels=1, out_channels=1, kernel_size=3, dropout=0.0, dropout_rate=0.0, bias=True,
                  use_causal_conv=False, upsample_conditional_features=True, upsample_net="ConvInUpsampleNetwork")


class ParallelWaveGANGeneratorHIP(_WaveGeneratorHIP):
    """compute="f32" (default): exact fp32 products.  compute="f16": the residual blocks run on the 16-bit MFMA, one launch per
    block (pwg_fused_f16.hip): the conv input, the upsampled mel, the gate output and the block weights are rounded to fp16
    (nearest even, saturated), everything else stays fp32.  It needs the fused v1 channel plan."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", layers=30, stacks=3, residual_channels=64,
                 gate_channels=128, skip_channels=64, aux_channels=80, aux_context_window=2,
                 upsample_scales: Sequence[int] = (4, 5, 3, 5), stats: Optional[Dict[str, np.ndarray]] = None,
                 fused: Optional[bool] = None, compute: str = "f32"):
        self.compute = _check_compute(compute)
        if compute == "f16":
            if (residual_channels, gate_channels, skip_channels, aux_channels) != (64, 128, 64, 80):
                raise ValueError("compute='f16' needs the v1 channel plan: 64 residual / 128 gate / 64 skip / 80 aux channels")
            if fused is not None and not fused:
                raise ValueError("compute='f16' is a mode of the fused residual blocks: fused=False cannot be combined with it")
            fused = True
        self._setup(device, aux_channels, stats, state_dict)
        self.layers, self.stacks = layers, stacks
        self.R, self.G, self.S = residual_channels, gate_channels, skip_channels
        self.ctx = aux_context_window
        self.scales = tuple(upsample_scales)
        self.upsample_factor = int(np.prod(self.scales))

        def w(p):
            return self._w(p).to(self.dev)

        self.w_first = w("first_conv").reshape(self.R, 1).contiguous()
        self.b_first = self._b("first_conv", self.R)
        self.w_in = _tap_major(w("upsample_net.conv_in"), self.dev)
        self.w_up = [w(f"upsample_net.upsample.up_layers.{2 * i + 1}").reshape(-1).contiguous() for i in range(len(self.scales))]
        # fused residual-block kernels (pwg_fused.hip) need the v1 channel plan: 64 residual / 128 gate / 64 skip / 80 aux
        if fused is None:
            fused = os.environ.get("A3T_PWG_FUSED", "1") != "0"
        self.fused = bool(fused) and (self.R, self.G, self.S, self.A) == (64, 128, 64, 80)
        self.blocks = []
        for l in range(layers):
            p = f"conv_layers.{l}."
            cw = w(p + "conv")
            blk = dict(w=_tap_major(cw, self.dev), b=self._b(p + "conv", self.G),
                       aux=w(p + "conv1x1_aux").reshape(self.G, self.A).contiguous(),
                       out=w(p + "conv1x1_out").reshape(self.R + self.S, self.G // 2).contiguous(),
                       bout=self._b(p + "conv1x1_out", self.R + self.S))
            if self.fused:      # wt0 [272][128] k-major in the gate permutation, wt1 [64][128]
                raw = (cw, blk["b"], blk["aux"], blk["out"])
                blk["wt0"], blk["b0"], blk["wt1"] = _pack_pwg_block(*raw)
                if compute == "f16":
                    blk["w0h"], blk["b0h"], blk["w1h"] = pack_pwg_block_f16(*raw)
            self.blocks.append(blk)
        self.w_l1 = w("last_conv_layers.1").reshape(self.S, self.S).contiguous()
        self.b_l1 = self._b("last_conv_layers.1", self.S)
        self.w_l3 = w("last_conv_layers.3").reshape(1, self.S).contiguous()
        self.b_l3 = self._b("last_conv_layers.3", 1)
        del self._sd

    @classmethod
    def from_config(cls, state_dict, generator_params: Dict, generator_type: str = "ParallelWaveGANGenerator", **kw):
        """From the `generator_params` (and `generator_type`) of a parallel_wavegan config.yml and the checkpoint's
        model["generator"] state dict.  kw: device, stats, fused, compute."""
        if generator_type != "ParallelWaveGANGenerator":
            raise NotImplementedError(f"generator_type {generator_type!r}: ParallelWaveGANGeneratorHIP builds ParallelWaveGANGenerator only")
        fixed = {k: (v, f"generator_params.{k}: only {v!r} is built into ParallelWaveGANGeneratorHIP") for k, v in _PWG_FIXED.items()}
        p = _config_params(dict(generator_params), _PWG_KNOWN, fixed)
        up = dict(p.pop("upsample_params", None) or {})
        if "upsample_scales" in up:
            p["upsample_scales"] = up.pop("upsample_scales")
        if up:
            raise NotImplementedError(f"generator_params.upsample_params {sorted(up)} are not understood")
        return cls(state_dict, **p, **kw)

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
        self._zero_tail(wav, lens, hop, B, Tw)
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
                self._zero_tail(x, lens, hop, B, Tw)

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
        self.compute = _check_compute(compute)
        if compute == "f16" and not fused:
            raise ValueError("compute='f16' is a mode of the fused kernels: it needs fused=True")
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
        self._setup(device, in_channels, stats, state_dict, bias)
        self.C0, self.K = int(channels), int(kernel_size)
        self.add, self.slope = bool(use_additional_convs), float(negative_slope)
        self.upsample_factor = int(np.prod(self.scales))
        w, b = self._w, self._b
        self.w_in, self.b_in = _tap_major(w("input_conv"), self.dev), b("input_conv", self.C0)
        if tuple(self.w_in.shape) != (self.C0, self.K, self.A):
            raise ValueError(f"input_conv.weight {tuple(self.w_in.shape)} does not fit channels / kernel_size / in_channels")
        self.stages = []
        for i, s in enumerate(self.scales):
            C = self.C0 >> (i + 1)
            f16 = compute == "f16" and C in F16_WIDTHS and max(self.rk) <= 11
            st = dict(C=C, s=s, f16=f16, w_up=pack_hifigan_upsample(w(f"upsamples.{i}.1"), s).to(self.dev),
                      b_up=b(f"upsamples.{i}.1", C, s),
                      fused=f16 or (bool(fused) and C in (32, 64) and max(self.rk) <= 11), blocks=[])
            for j, (k, dils) in enumerate(zip(self.rk, self.rd)):
                units = []
                for d in range(len(dils)):
                    p = f"blocks.{i * len(self.rk) + j}."
                    names = [p + f"convs1.{d}.1"] + ([p + f"convs2.{d}.1"] if self.add else [])
                    ws = [w(n) for n in names]
                    units.append(dict(dil=dils[d], b=[b(n, C) for n in names],
                                      w=[(pack_hifigan_conv_f16(t).to(self.dev) if f16 else
                                          pack_hifigan_conv(t).to(self.dev) if st["fused"] else _tap_major(t, self.dev)) for t in ws]))
                st["blocks"].append(dict(k=k, units=units))
            self.stages.append(st)
        Cl = self.C0 >> len(self.scales)
        w_out = w("output_conv.1")
        if tuple(w_out.shape) != (1, Cl, self.K):
            raise NotImplementedError(f"out_channels: output_conv.1.weight {tuple(w_out.shape)} is not (1, {Cl}, {self.K})")
        self.w_out = _tap_major(w_out, self.dev)                      # [1][K][Cl]
        self.b_out = b("output_conv.1", 1)
        self.fused_out = bool(fused) and Cl <= 64 and Cl % 4 == 0 and self.K <= 11
        self.fused = any(st["fused"] for st in self.stages)
        del self._sd

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
        ap = dict(p.pop("nonlinear_activation_params", None) or {"negative_slope": 0.1})
        if "upsample_kernal_sizes" in p:    # (the zoo's older configs spell it so)
            p["upsample_kernel_sizes"] = p.pop("upsample_kernal_sizes")
        known = ("in_channels", "channels", "kernel_size", "upsample_scales", "upsample_kernel_sizes", "resblock_kernel_sizes",
                 "resblock_dilations", "use_additional_convs", "bias")
        p = _config_params(p, known, dict(nonlinear_activation=_LRELU_ONLY, use_causal_conv=_NOT_CAUSAL))
        return cls(state_dict, negative_slope=float(ap.get("negative_slope", 0.01)), **p, **kw)

    @property
    def margin_frames(self) -> int:
        return hifigan_margin_frames(self.scales, self.rk, self.rd, self.K, self.add)

    @torch.no_grad()
    def inference(self, c: torch.Tensor, z: Optional[torch.Tensor] = None, normalize_before: bool = False,
                  lengths: Optional[Sequence[int]] = None):
        """c (T_feats, aux) [or (B, T_feats, aux)] -> (T_wav, 1) [or (B, T_wav, 1)]; z must be None (HiFi-GAN has no noise input).

        lengths (host integers, one per row of a (B, Tmax, aux) batch): row b is computed exactly as if c[b, :L_b] had been
        passed alone -- every convolution reads zeros behind the row's end at its own rate and stores zeros there -- and the
        result (B, Tmax * hop, 1) is zero behind L_b * hop.  What the padding of c holds reaches no valid sample."""
        if z is not None:
            raise ValueError("HiFiGANGeneratorHIP.inference: z must be None, the HiFi-GAN generator has no noise input")
        c, single, lens, tiles = self.prepare(c, normalize_before, lengths, self._tiled_rates((1,) if self.fused_out else ()))
        B, Tf, A = c.shape
        dev = self.dev
        c = self._ragged_copy(c, lens)
        x = torch.empty(B * Tf, self.C0, device=dev)
        ops.conv_fwd(c.view(B * Tf, A), self.w_in, x, Tf, (self.K - 1) // 2, bias=self.b_in, compute=F32)
        self._zero_tail(x, lens, 1, B, Tf)
        T, rate = Tf, 1
        for st in self.stages:
            up = self._upsample(x, st["w_up"], st["b_up"], B, T, st["s"], st["C"], lens, rate, self.slope)
            T, rate = T * st["s"], rate * st["s"]
            run = self._stage_fused if st["fused"] else self._stage_layers
            x = run(st, up, B, T, rate, lens, tiles.get(rate))
        wav = torch.empty(B * T, 1, device=dev)
        if self.fused_out:
            if lens is not None:      # the kernel writes no sample behind a row's end
                wav.zero_()
            ops.hfg_out(x, self.w_out.view(self.K, -1), self.b_out, wav, B, T, 0.01, tiles.get(rate))
        else:
            ops.conv_fwd(self._lrelu(x, 0.01), self.w_out, wav, T, (self.K - 1) // 2, bias=self.b_out, act=ACT_TANH, compute=F32)
            self._zero_tail(wav, lens, rate, B, T)
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
                    self._zero_tail(xt, lens, rate, B, T)
                    ops.conv_fwd(self._lrelu(xt), unit["w"][1], xn, T, pad, 1, bias=unit["b"][1], R=x, compute=F32)
                else:
                    ops.conv_fwd(self._lrelu(x), unit["w"][0], xn, T, pad, unit["dil"], bias=unit["b"][0], R=x, compute=F32)
                self._zero_tail(xn, lens, rate, B, T)
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


# ------------------------------------------------------------------------------- MelGAN / multi-band MelGAN generator
def melgan_margin_frames(upsample_scales: Sequence[int] = (5, 5, 3), stacks: int = 4, stack_kernel_size: int = 3,
                         kernel_size: int = 7, out_channels: int = 4, pqmf_taps: int = 62) -> int:
    """pwg_margin_frames for the MelGAN generator, walked from the output back to the mel like hifigan_margin_frames: the PQMF
    synthesis filter reaches ceil((taps / 2) / subbands) sub-band samples (multi-band only), the output convolution (K-1)/2; the
    residual stacks of a stage sum_j (ks-1)/2 * ks^j of its samples (their 1x1 convolutions none); a transposed convolution of
    scale s turns a reach of n into ceil(n / s) + 1; the input convolution adds (K-1)/2 frames.  Reflection does not widen the
    reach: it happens at an utterance's ends only, which a clipped window shares.  15 for the multi-band v2 plan."""
    S, ks = int(out_channels), int(stack_kernel_size)
    n = -(-(int(pqmf_taps) // 2) // S) if S > 1 else 0
    n += (int(kernel_size) - 1) // 2
    reach = sum((ks - 1) // 2 * ks ** j for j in range(int(stacks)))
    for s in reversed([int(s) for s in upsample_scales]):
        n = -(-(n + reach) // s) + 1
    return n + (int(kernel_size) - 1) // 2


def melgan_min_frames(upsample_scales: Sequence[int] = (5, 5, 3), stacks: int = 4, stack_kernel_size: int = 3,
                      kernel_size: int = 7) -> int:
    """The smallest number of frames for which every reflection of the plan is legal (ReflectionPad1d needs pad < length): the
    input convolution pads (K-1)/2 frames, the widest stack of stage i (ks-1)/2 * ks^(stacks-1) samples at prod(scales[:i+1])
    samples per frame, the output convolution (K-1)/2 samples at the last rate.  6 for the v2 plan."""
    half, ks = (int(kernel_size) - 1) // 2, int(stack_kernel_size)
    need, rate = half + 1, 1
    dmax = (ks - 1) // 2 * ks ** (int(stacks) - 1) if stacks else 0
    for s in upsample_scales:
        rate *= int(s)
        need = max(need, dmax // rate + 1)
    return max(need, half // rate + 1)


def pqmf_synthesis_filter(subbands: int = 4, taps: int = 62, cutoff_ratio: float = 0.142, beta: float = 9.0) -> np.ndarray:
    """The synthesis filters [subbands][taps + 1] of the reference's PQMF (pqmf.py:17-53, 88-115: a Kaiser-windowed sinc prototype,
    cosine modulated), computed in fp64 with numpy alone and rounded to fp32 -- the precision the reference holds them in, also in
    its .double() model."""
    if taps % 2 or not 0.0 < cutoff_ratio < 1.0:
        raise ValueError("pqmf: taps must be even and 0 < cutoff_ratio < 1")
    n = np.arange(taps + 1) - 0.5 * taps
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.sin(np.pi * cutoff_ratio * n) / (np.pi * n)
    h[taps // 2] = np.cos(0) * cutoff_ratio
    h = h * np.kaiser(taps + 1, beta)
    out = np.zeros((subbands, taps + 1))
    for k in range(subbands):
        out[k] = 2 * h * np.cos((2 * k + 1) * (np.pi / (2 * subbands)) * (np.arange(taps + 1) - (taps / 2)) - (-1) ** k * np.pi / 4)
    return out.astype(np.float32)


MGAN_WIDTHS = (48, 96, 192)      # the stage widths a3t_mgan_stack is built for


def melgan_hidden_order(Cp: int) -> np.ndarray:
    """Hidden channel of row 16 q + 2 kk + lk of a3t_mgan_stack's W2 operand: the channel that register r = 8 (q & 1) + kk of
    accumulator block q >> 1 holds in lane half lk."""
    row = np.arange(Cp)
    q, kk, lk = row // 16, (row % 16) // 2, row % 2
    r = 8 * (q & 1) + kk
    return 32 * (q >> 1) + (r & 3) + 8 * (r >> 2) + 4 * lk


def pack_melgan_stack(w1, b1, w2, b2, ws, bs):
    """Operands of a3t_mgan_stack from one ResidualStack's parameters (pure; CPU or device tensors): w1 [C][C][3] dilated conv,
    w2 [C][C][1] and ws [C][C][1] (skip_layer), biases [C] or None -> w [4 C + Cp][Cp] (Cp = C rounded up to 32): rows tap*C + in
    channel of w1, then the in channels of ws, then Cp rows of w2 in melgan_hidden_order, columns = out channels, zero where a
    row or column is >= C;  bias [2][Cp] = b1 | bs + b2, zero-padded."""
    w1 = torch.as_tensor(w1, dtype=torch.float32)
    C = w1.shape[0]
    if tuple(w1.shape) != (C, C, 3) or tuple(w2.shape) != (C, C, 1) or tuple(ws.shape) != (C, C, 1) or C % 16:
        raise ValueError(f"pack_melgan_stack: weights {tuple(w1.shape)} / {tuple(w2.shape)} / {tuple(ws.shape)} are not a "
                         "ResidualStack of kernel size 3 and a width that is a multiple of 16")
    Cp = (C + 31) // 32 * 32
    dev = w1.device
    w = torch.zeros(4 * C + Cp, Cp, dtype=torch.float32, device=dev)
    w[:3 * C, :C] = w1.permute(2, 1, 0).reshape(3 * C, C)
    w[3 * C:4 * C, :C] = torch.as_tensor(ws, dtype=torch.float32).to(dev)[:, :, 0].t()
    w2t = torch.zeros(Cp, Cp, dtype=torch.float32, device=dev)
    w2t[:C, :C] = torch.as_tensor(w2, dtype=torch.float32).to(dev)[:, :, 0].t()      # [hidden][out]
    w[4 * C:] = w2t[torch.as_tensor(melgan_hidden_order(Cp), device=dev)]
    bias = torch.zeros(2, Cp, dtype=torch.float32, device=dev)
    if b1 is not None:
        bias[0, :C] = torch.as_tensor(b1, dtype=torch.float32).to(dev)
    for v in (bs, b2):
        if v is not None:
            bias[1, :C] += torch.as_tensor(v, dtype=torch.float32).to(dev)
    return w.contiguous(), bias


class MelGANGeneratorHIP(_WaveGeneratorHIP):
    """MelGAN / multi-band MelGAN generator inference (espnet2/gan_tts/melgan/melgan.py:22-199, residual_stack.py:16-71,
    pqmf.py:56-160; state-dict compatible with the parallel_wavegan zoo's MelGANGenerator), channels-last fp32 [B*T][C] on the
    device.  Every non-transposed convolution reflects at the ends of the row it belongs to (ReflectionPad1d), so an input needs
    min_frames frames; out_channels > 1 is the multi-band form, whose sub-bands the PQMF synthesis filter bank (a3t_pqmf_synthesis)
    turns into the waveform: upsample_factor = prod(upsample_scales) * out_channels.

    fused=False: layer by layer -- a3t_leaky_relu, a3t_reflect_pad_rows, the convolution on the exact-fp32 GEMM over the padded
    rows, the interior sliced out.  fused=True: the residual stacks of the stages whose width is in MGAN_WIDTHS run on
    a3t_mgan_stack, one launch each, and the output convolution on a3t_mgan_out where it fits (C <= 64, out_channels <= 4,
    K <= 11); the rest runs layer by layer.  fused=True is the default because it is the faster path on the v2 plan
    (profiles/melgan_latency.txt: 4.3 ms against 11.3 ms for 8 x 1000 frames)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", in_channels=80, out_channels=4, kernel_size=7,
                 channels=384, upsample_scales: Sequence[int] = (5, 5, 3), stack_kernel_size=3, stacks=4, bias=True,
                 negative_slope=0.2, use_final_nonlinear_activation=True, pqmf: Optional[Dict] = None,
                 stats: Optional[Dict[str, np.ndarray]] = None, fused=True):
        self.scales = tuple(int(s) for s in upsample_scales)
        self.K, self.ks, self.nstacks, self.O = int(kernel_size), int(stack_kernel_size), int(stacks), int(out_channels)
        if self.K % 2 == 0 or self.ks % 2 == 0:
            raise ValueError(f"kernel_size {kernel_size} and stack_kernel_size {stack_kernel_size} must be odd")
        if channels % (2 ** len(self.scales)):
            raise ValueError(f"channels {channels} must be divisible by 2^{len(self.scales)}")
        if self.O < 1:
            raise ValueError(f"out_channels {out_channels} must be positive")
        self._setup(device, in_channels, stats, state_dict, bias)
        self.C0, self.slope, self.final_tanh = int(channels), float(negative_slope), bool(use_final_nonlinear_activation)
        self.upsample_factor = int(np.prod(self.scales)) * self.O
        self.pqmf = dict(dict(taps=62, cutoff_ratio=0.142, beta=9.0), **(pqmf or {})) if self.O > 1 else None
        if self.pqmf is not None:
            if self.O > 8 or self.pqmf["taps"] > 254:
                raise NotImplementedError(f"pqmf: {self.O} sub-bands / {self.pqmf['taps']} taps: a3t_pqmf_synthesis is built for <= 8 / <= 254")
            self.h_syn = torch.from_numpy(pqmf_synthesis_filter(self.O, **self.pqmf)).to(self.dev)
        self.min_frames = melgan_min_frames(self.scales, self.nstacks, self.ks, self.K)
        w, b = self._w, self._b
        # the reference's Sequential: 0 pad, 1 conv | per stage: activation, transposed conv, `stacks` ResidualStacks | activation,
        # pad, conv (, tanh)
        self.w_in, self.b_in = _tap_major(w("melgan.1"), self.dev), b("melgan.1", self.C0)
        if tuple(self.w_in.shape) != (self.C0, self.K, self.A):
            raise ValueError(f"melgan.1.weight {tuple(self.w_in.shape)} does not fit channels / kernel_size / in_channels")
        self.stages, idx = [], 2
        for i, s in enumerate(self.scales):
            C = self.C0 >> (i + 1)
            st = dict(C=C, s=s, fused=bool(fused) and C in MGAN_WIDTHS and self.ks == 3, stacks=[],
                      w_up=pack_hifigan_upsample(w(f"melgan.{idx + 1}"), s).to(self.dev), b_up=b(f"melgan.{idx + 1}", C, s))
            for j in range(self.nstacks):
                p = f"melgan.{idx + 2 + j}."
                raw = (w(p + "stack.2"), b(p + "stack.2", C), w(p + "stack.4"), b(p + "stack.4", C), w(p + "skip_layer"),
                       b(p + "skip_layer", C))
                if tuple(raw[0].shape) != (C, C, self.ks):
                    raise ValueError(f"{p}stack.2.weight {tuple(raw[0].shape)} is not ({C}, {C}, {self.ks})")
                unit = dict(dil=self.ks ** j)
                if st["fused"]:
                    unit["w"], unit["b"] = (t.to(self.dev) for t in pack_melgan_stack(*raw))
                else:
                    unit.update(w1=_tap_major(raw[0], self.dev), b1=raw[1], w2=raw[2].reshape(C, C).contiguous().to(self.dev), b2=raw[3],
                                ws=raw[4].reshape(C, C).contiguous().to(self.dev), bs=raw[5])
                st["stacks"].append(unit)
            self.stages.append(st)
            idx += 2 + self.nstacks
        Cl = self.C0 >> len(self.scales)
        self.w_out, self.b_out = _tap_major(w(f"melgan.{idx + 2}"), self.dev), b(f"melgan.{idx + 2}", self.O)      # [O][K][Cl]
        if tuple(self.w_out.shape) != (self.O, self.K, Cl):
            raise ValueError(f"melgan.{idx + 2}.weight {tuple(self.w_out.shape)} does not fit out_channels / kernel_size / channels")
        self.fused_out = bool(fused) and Cl <= 64 and Cl % 2 == 0 and self.O <= 4 and self.K <= 11
        self.fused = self.fused_out or any(st["fused"] for st in self.stages)
        del self._sd

    @classmethod
    def from_config(cls, state_dict, generator_params: Dict, generator_type: str = "MelGANGenerator",
                    pqmf_params: Optional[Dict] = None, **kw):
        """From the `generator_params`, `generator_type` and `pqmf_params` of a parallel_wavegan config.yml and the checkpoint's
        model["generator"] state dict.  kw: device, stats, fused."""
        if generator_type != "MelGANGenerator":
            raise NotImplementedError(f"generator_type {generator_type!r}: MelGANGeneratorHIP builds MelGANGenerator only")
        p = dict(generator_params)
        if p.pop("pad_params", None):
            raise NotImplementedError("pad_params must be empty (ReflectionPad1d takes none)")
        ap = dict(p.pop("nonlinear_activation_params", None) or {"negative_slope": 0.2})
        known = ("in_channels", "out_channels", "kernel_size", "channels", "upsample_scales", "stack_kernel_size", "stacks", "bias",
                 "use_final_nonlinear_activation")
        fixed = dict(pad=("ReflectionPad1d", "pad {!r}: only ReflectionPad1d is built into the kernels"),
                     nonlinear_activation=_LRELU_ONLY, use_causal_conv=_NOT_CAUSAL)
        p = _config_params(p, known, fixed)
        p.setdefault("out_channels", 1)      # (the reference constructor's defaults, where they differ from this class's)
        p.setdefault("channels", 512)
        p.setdefault("upsample_scales", [8, 8, 2, 2])
        p.setdefault("stacks", 3)
        pq = dict(pqmf_params or {})
        if int(pq.pop("subbands", p["out_channels"])) != int(p["out_channels"]) and int(p["out_channels"]) > 1:
            raise NotImplementedError("pqmf_params.subbands must equal generator_params.out_channels")
        bad = sorted(set(pq) - {"taps", "cutoff_ratio", "beta"})
        if bad:
            raise NotImplementedError(f"pqmf_params {bad} are not understood")
        return cls(state_dict, negative_slope=float(ap.get("negative_slope", 0.01)), pqmf=pq, **p, **kw)

    @property
    def margin_frames(self) -> int:
        return melgan_margin_frames(self.scales, self.nstacks, self.ks, self.K, self.O, self.pqmf["taps"] if self.pqmf else 0)

    @torch.no_grad()
    def inference(self, c: torch.Tensor, z: Optional[torch.Tensor] = None, normalize_before: bool = False,
                  lengths: Optional[Sequence[int]] = None):
        """c (T_feats, aux) [or (B, T_feats, aux)] -> (T_wav, 1) [or (B, T_wav, 1)]; z must be None (MelGAN has no noise input).

        lengths (host integers, one per row of a (B, Tmax, aux) batch): row b is computed exactly as if c[b, :L_b] had been
        passed alone -- every reflection happens at the row's own ends at that layer's rate, the transposed convolutions and the
        PQMF filter read zeros behind them -- and the result (B, Tmax * hop, 1) is zero behind L_b * hop.  What the padding of c
        holds reaches no valid sample.  An input, or a row that is not empty, needs min_frames frames (ValueError)."""
        if z is not None:
            raise ValueError("MelGANGeneratorHIP.inference: z must be None, the MelGAN generator has no noise input")
        rows = [int(n) for n in lengths] if lengths is not None else [c.shape[-2]]
        short = [n for n in rows if n < self.min_frames and (n > 0 or lengths is None)]      # (a length of 0 is an empty row)
        if short:
            raise ValueError(f"MelGANGeneratorHIP.inference: {short[0]} frames are fewer than min_frames = {self.min_frames} "
                             "(a reflection must be shorter than the signal it pads)")
        rates = self._tiled_rates(((1,) if self.fused_out else ()) + ((self.O,) if self.pqmf is not None else ()))
        c, single, lens, tiles = self.prepare(c, normalize_before, lengths, rates)
        B, Tf, A = c.shape
        dev, half = self.dev, (self.K - 1) // 2
        Lmin = min([int(n) for n in lengths if int(n) > 0], default=Tf) if lengths is not None else Tf

        def buf(T, C):      # the tiled kernels write nothing behind a row's end: what reads it next finds zeros there
            return (torch.zeros if lens is not None else torch.empty)(B * T, C, device=dev)

        c = self._ragged_copy(c, lens)
        x = self._conv_reflect(c.view(B * Tf, A), self.w_in, self.b_in, B, Tf, half, 1, lens, 1)
        self._zero_tail(x, lens, 1, B, Tf)
        T, rate = Tf, 1
        for st in self.stages:
            C = st["C"]
            x = self._upsample(x, st["w_up"], st["b_up"], B, T, st["s"], C, lens, rate, self.slope)
            T, rate = T * st["s"], rate * st["s"]
            pp = [buf(T, C), buf(T, C)] if st["fused"] else None
            for j, u in enumerate(st["stacks"]):
                if st["fused"]:
                    ops.mgan_stack(x, u["w"], u["b"], pp[j % 2], B, T, u["dil"], self.slope, tiles.get(rate), Lmin * rate)
                    x = pp[j % 2]
                else:
                    x = self._stack_layers(u, x, B, T, rate, lens)
            if not st["fused"]:
                self._zero_tail(x, lens, rate, B, T)
        if self.fused_out:
            y = buf(T, self.O)
            ops.mgan_out(x, self.w_out, self.b_out, y, B, T, self.slope, self.final_tanh, tiles.get(rate), Lmin * rate)
        else:
            y = self._conv_reflect(self._lrelu(x), self.w_out, self.b_out, B, T, half, 1, lens, rate,
                                   ACT_TANH if self.final_tanh else 0)
            self._zero_tail(y, lens, rate, B, T)
        if self.pqmf is not None:
            wav = buf(T * self.O, 1)
            ops.pqmf_synthesis(y, self.h_syn, wav, B, T, tiles.get(rate * self.O))
            T *= self.O
        else:
            wav = y
        wav = wav.view(B, T, 1)
        return wav[0] if single else wav

    def _conv_reflect(self, x, w, bias, B, T, half, dil, lens, rate, act=0):
        """conv(reflect_pad(x)) layer by layer, the convolution of 2 half + 1 taps at dilation dil: x [B*T][Cin] is padded by
        half * dil rows at each row's own ends, convolved on the exact-fp32 GEMM over the padded rows and the interior sliced out
        -> [B*T][Cout]."""
        pad = half * dil
        Tp, N = T + 2 * pad, w.shape[0]
        xp = torch.empty(B * Tp, x.shape[1], device=self.dev)
        ops.reflect_pad_rows(x.view(B, T, -1), xp, pad, lens, rate)
        yp = torch.empty(B * Tp, N, device=self.dev)
        ops.conv_fwd(xp, w, yp, Tp, half, dil, bias=bias, act=act, compute=F32)
        return yp.view(B, Tp, N)[:, pad:pad + T].reshape(B * T, N)

    def _stack_layers(self, u, x, B, T, rate, lens):
        """One ResidualStack layer by layer: skip_1x1(x) + conv_1x1(leaky(conv_dilated(reflect_pad(leaky(x)))))."""
        C = x.shape[1]
        h = self._conv_reflect(self._lrelu(x), u["w1"], u["b1"], B, T, (self.ks - 1) // 2, u["dil"], lens, rate)
        sk = torch.empty(B * T, C, device=self.dev)
        ops.linear_fwd(x, u["ws"], sk, bias=u["bs"], compute=F32)
        y = torch.empty(B * T, C, device=self.dev)
        ops.linear_fwd(self._lrelu(h), u["w2"], y, bias=u["b2"], R=sk, compute=F32)
        return y

    __call__ = inference


# ------------------------------------------------------------------------------------------------ StyleMelGAN generator
class StyleMelGANGeneratorHIP(_WaveGeneratorHIP):
    """StyleMelGAN generator inference (espnet2/gan_tts/style_melgan/style_melgan.py:28-232, tade_res_block.py:15-185; state-dict
    compatible with the parallel_wavegan zoo's StyleMelGANGenerator, weight norm folded at load), channels-last fp32 [B*T][C] on
    the device.  The defaults are the zoo's 24 kHz plan (hop 300).

    The noise z has ceil(T / F) steps of in_channels (F = noise_upsample_factor), which the transposed convolutions
    (pack_hifigan_upsample on the exact-fp32 GEMM, a3t_leaky_relu) bring to n_eff = ceil(T / F) * F frames of `channels`; c is
    padded to n_eff frames with its last frame, the network runs over n_eff * hop samples and the output is cut to T * hop
    (style_melgan.py:208-230).  A TADEResBlock is six a3t_smg_conv launches (nearest-neighbour upsampling is an index map inside
    them) and two a3t_smg_stats; the output convolution is a3t_hfg_out with slope 1.

    InstanceNorm1d takes its statistics over the whole time axis, so every sample depends on the whole utterance:
    margin_frames is None (there is no finite margin, SpeechEditor vocodes whole utterances) and min_frames is 1."""

    min_frames = 1
    margin_frames = None

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", in_channels=128, aux_channels=80, channels=64,
                 out_channels=1, kernel_size=9, dilation=2, bias=True, noise_upsample_scales: Sequence[int] = (10, 2, 2, 2),
                 noise_upsample_negative_slope=0.2, upsample_scales: Sequence[int] = (5, 1, 5, 1, 3, 1, 2, 2, 1),
                 gated_function="softmax", stats: Optional[Dict[str, np.ndarray]] = None):
        if int(channels) != 64:
            raise NotImplementedError(f"channels {channels}: a3t_smg_conv is built for 64 channels")
        if int(out_channels) != 1:
            raise NotImplementedError(f"out_channels {out_channels}: only 1 is built here")
        if gated_function not in ("softmax", "sigmoid"):
            raise NotImplementedError(f"gated_function {gated_function!r}: softmax and sigmoid are built into a3t_smg_conv")
        if int(kernel_size) % 2 == 0 or int(kernel_size) > 9 or int(kernel_size) < 1:
            raise NotImplementedError(f"kernel_size {kernel_size}: a3t_smg_conv takes an odd kernel size up to 9")
        if int(in_channels) % 16 or int(in_channels) < 16:
            raise NotImplementedError(f"in_channels {in_channels} must be a multiple of 16")
        if int(aux_channels) % 16 or int(aux_channels) < 16:
            raise NotImplementedError(f"aux_channels {aux_channels} must be a multiple of 16")
        self.noise_scales = tuple(int(s) for s in noise_upsample_scales)
        self.scales = tuple(int(s) for s in upsample_scales)
        if any(s == 1 for s in self.noise_scales):      # (output_padding = s % 2 must be smaller than the stride)
            raise NotImplementedError(f"noise_upsample_scales {list(self.noise_scales)}: a scale of 1 is a transposed convolution "
                                      "the reference cannot run either")
        if any(s < 1 for s in self.noise_scales + self.scales) or int(dilation) < 1:
            raise ValueError("scales and dilation must be positive")
        self._setup(device, aux_channels, stats, state_dict, bias)
        self.Z, self.C, self.K, self.dil = int(in_channels), 64, int(kernel_size), int(dilation)
        self.noise_slope, self.sigmoid = float(noise_upsample_negative_slope), gated_function == "sigmoid"
        self.noise_upsample_factor = int(np.prod(self.noise_scales))
        self.hop = self.upsample_factor = int(np.prod(self.scales))

        w, b = self._w, self._b

        def conv(p, cout, cin):      # Conv1d [cout][cin][K] -> the k-major operand [K*cin][cout]
            t = w(p)
            if tuple(t.shape) != (cout, cin, self.K):
                raise ValueError(f"{p}.weight {tuple(t.shape)} is not ({cout}, {cin}, {self.K})")
            return pack_hifigan_conv(t).to(self.dev), b(p, cout)

        self.noise = []
        for i, s in enumerate(self.noise_scales):
            p, cin = f"noise_upsample.{2 * i}", self.Z if i == 0 else self.C
            t = w(p)
            if tuple(t.shape) != (cin, self.C, 2 * s):
                raise ValueError(f"{p}.weight {tuple(t.shape)} is not ({cin}, {self.C}, {2 * s})")
            self.noise.append(dict(s=s, w=pack_hifigan_upsample(t, s).to(self.dev), b=b(p, self.C, s)))
        self.blocks = []
        for k, u in enumerate(self.scales):
            p, aux = f"blocks.{k}.", self.A if k == 0 else self.C
            self.blocks.append(dict(u=u, aux1=conv(p + "tade1.aux_conv.0", 64, aux), tade1=conv(p + "tade1.gated_conv.0", 128, 64),
                                    gate1=conv(p + "gated_conv1", 128, 64), aux2=conv(p + "tade2.aux_conv.0", 64, 64),
                                    tade2=conv(p + "tade2.gated_conv.0", 128, 64), gate2=conv(p + "gated_conv2", 128, 64)))
        w_out = w("output_conv.0")
        if tuple(w_out.shape) != (1, self.C, self.K):
            raise ValueError(f"output_conv.0.weight {tuple(w_out.shape)} is not (1, {self.C}, {self.K})")
        self.w_out = w_out[0].t().contiguous().to(self.dev)      # [K][C]
        self.b_out = b("output_conv.0", 1)
        del self._sd

    @classmethod
    def from_config(cls, state_dict, generator_params: Dict, generator_type: str = "StyleMelGANGenerator", **kw):
        """From the `generator_params` (and `generator_type`) of a parallel_wavegan config.yml and the checkpoint's
        model["generator"] state dict.  kw: device, stats."""
        if generator_type != "StyleMelGANGenerator":
            raise NotImplementedError(f"generator_type {generator_type!r}: StyleMelGANGeneratorHIP builds StyleMelGANGenerator only")
        p = dict(generator_params)
        ap = p.pop("noise_upsample_activation_params", None)
        ap = {"negative_slope": 0.2} if ap is None else dict(ap)      # (given but empty: torch's own default, 0.01)
        known = ("in_channels", "aux_channels", "channels", "out_channels", "kernel_size", "dilation", "bias", "noise_upsample_scales",
                 "upsample_scales", "gated_function")
        fixed = dict(upsample_mode=("nearest", "upsample_mode {!r}: only nearest is built into a3t_smg_conv"),
                     noise_upsample_activation=("LeakyReLU", "noise_upsample_activation {!r}: only LeakyReLU is built here"))
        p = _config_params(p, known, fixed)
        p.setdefault("noise_upsample_scales", [11, 2, 2, 2])      # (the reference constructor's defaults, where they differ)
        p.setdefault("upsample_scales", [2, 2, 2, 2, 2, 2, 2, 2, 1])
        return cls(state_dict, noise_upsample_negative_slope=float(ap.get("negative_slope", 0.01)), **p, **kw)

    def noise_shape(self, frames: int):
        """The shape of the noise z that `frames` frames take: (ceil(frames / F), in_channels)."""
        return (-(-int(frames) // self.noise_upsample_factor), self.Z)

    @torch.no_grad()
    def inference(self, c: torch.Tensor, z: Optional[torch.Tensor] = None, normalize_before: bool = False,
                  lengths: Optional[Sequence[int]] = None):
        """c (T_feats, aux) [or (B, T_feats, aux)], z (m, in_channels) [or (B, m, in_channels)] with m = ceil(T_feats / F), or
        None for torch.randn on the device -> (T_wav, 1) [or (B, T_wav, 1)].

        lengths (host integers, one per row of a (B, Tmax, aux) batch): row b is computed exactly as if c[b, :L_b] and
        z[b, :ceil(L_b / F)] had been passed alone: its network length is n_eff_b = ceil(L_b / F) * F frames, its c is padded to
        that with its own last frame, every convolution reads zeros outside [0, n_eff_b * rate), every InstanceNorm statistic runs
        over the row's own n_eff_b * rate samples, and the result (B, Tmax * hop, 1) is zero behind L_b * hop.  What the padding of
        c and z holds reaches no valid sample."""
        F, hop, dev = self.noise_upsample_factor, self.hop, self.dev
        c, single, rows = self._check_input(c, normalize_before, lengths)
        B, Tf, A = c.shape
        if Tf < 1:
            raise ValueError("StyleMelGANGeneratorHIP.inference: c has no frames")
        if rows is None:
            rows = [Tf] * B
        msteps = [-(-n // F) for n in rows]
        M = -(-Tf // F)
        Te = M * F
        want = (M, self.Z) if single else (B, M, self.Z)
        if z is None:
            z = torch.randn(B, M, self.Z, device=dev)
        elif tuple(z.shape) != want:
            raise ValueError(f"z has shape {tuple(z.shape)}, expected {want}: ceil({Tf} / {F}) steps of {self.Z} channels")
        x = z.to(dev, torch.float32).reshape(B * M, self.Z).contiguous()
        rates = sorted(set(np.cumprod((1,) + self.scales).tolist()))
        lens = mlen = None
        tiles = {}
        if lengths is not None:      # lengths | noise steps | one tile list of the n_eff per rate
            (lens, mlen), tiles = self._pack_meta([rows, msteps], [m * F for m in msteps], rates)
            x = x.clone()
            ops.zero_tail(x, mlen, 1, B, M)
        # ---- c padded to n_eff frames with each row's own last frame (a gather of frame indices)
        last = torch.as_tensor([max(n - 1, 0) for n in rows], device=dev)
        idx = torch.minimum(torch.arange(Te, device=dev)[None], last[:, None])
        cc = c.gather(1, idx[:, :, None].expand(B, Te, A)).contiguous().view(B * Te, A)
        # ---- noise path: transposed convolutions as 3-tap convolutions, LeakyReLU behind each
        T = M
        for st in self.noise:
            x = self._upsample(x, st["w"], st["b"], B, T, st["s"], self.C, mlen, T // M, self.noise_slope, after=True)
            T *= st["s"]
        # ---- TADEResBlocks
        rate = 1
        for blk in self.blocks:
            x, cc, rate = self._block(blk, x, cc, B, Te, rate, tiles)
        Tw = Te * hop
        wav = (torch.zeros if lens is not None else torch.empty)(B * Tw, 1, device=dev)
        ops.hfg_out(x, self.w_out, self.b_out, wav, B, Tw, 1.0, tiles.get(hop))      # slope 1: no activation in front
        self._zero_tail(wav, lens, hop, B, Tw)
        wav = wav.view(B, Tw, 1)[:, :Tf * hop]
        return wav[0] if single else wav.contiguous()

    def _block(self, blk, x, c, B, Te, rate, tiles):
        """One TADEResBlock: x, c [B * Te * rate][.] -> (x, c) [B * Te * rate * u][64], the new rate."""
        dev, u, sg = self.dev, blk["u"], self.sigmoid
        T1, T2 = Te * rate, Te * rate * u
        t1, t2 = tiles.get(rate), tiles.get(rate * u)

        def e(T):
            return torch.empty(B * T, 64, device=dev)

        st = torch.empty(2, B, 2, 64, device=dev)
        part = torch.empty(128 * B * ((T1 + 255) // 256), device=dev)
        ops.smg_stats(x, st[0], B, T1, t1, part=part)
        c1, y1, g1 = e(T1), e(T1), e(T1)
        ops.smg_conv(c, *blk["aux1"], c1, B, T1, tiles=t1)
        ops.smg_conv(c1, *blk["tade1"], y1, B, T1, mode=ops.SMG_TADE, m=x, stats=st[0], tiles=t1)
        ops.smg_conv(y1, *blk["gate1"], g1, B, T1, mode=ops.SMG_GATE, sigmoid=sg, tiles=t1)
        ops.smg_stats(g1, st[1], B, T1, t1, part=part)
        c2, y2, out = e(T2), e(T2), e(T2)
        ops.smg_conv(c1, *blk["aux2"], c2, B, T2, up=u, tiles=t2)
        ops.smg_conv(c2, *blk["tade2"], y2, B, T2, mode=ops.SMG_TADE, m=g1, stats=st[1], ux=u, tiles=t2)
        ops.smg_conv(y2, *blk["gate2"], out, B, T2, dil=self.dil, mode=ops.SMG_GATE, R=x, ur=u, sigmoid=sg, tiles=t2)
        return out, c2, rate * u

    __call__ = inference


# ------------------------------------------------------------------------------------------ a generator from a config
def generator_from_config(state_dict, config: Dict, **kw):
    """The generator class of a parallel_wavegan checkpoint's config (the dict of its config.yml: generator_type,
    generator_params and, for multi-band MelGAN, pqmf_params) over the checkpoint's model["generator"] state dict: what the
    reference driver's load_vocoder(tag) does once the files are on disk.  kw: device, stats, fused (and compute, where the class
    has it)."""
    gtype = config.get("generator_type", "ParallelWaveGANGenerator")
    classes = dict(ParallelWaveGANGenerator=ParallelWaveGANGeneratorHIP, HiFiGANGenerator=HiFiGANGeneratorHIP,
                   MelGANGenerator=MelGANGeneratorHIP)
    if gtype not in classes:
        raise NotImplementedError(f"generator_type {gtype!r}: ParallelWaveGANGenerator, HiFiGANGenerator and MelGANGenerator are built here"
                                  + (" (a StyleMelGANGenerator: StyleMelGANGeneratorHIP.from_config)" if gtype == "StyleMelGANGenerator" else ""))
    if gtype == "MelGANGenerator":
        kw = dict(kw, pqmf_params=config.get("pqmf_params"))
    return classes[gtype].from_config(state_dict, dict(config.get("generator_params") or {}), gtype, **kw)
