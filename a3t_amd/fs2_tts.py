"""Conformer FastSpeech2 as a TTS model on the device: text to mel, the TTS baselines of the speech-editing driver.

The reference runs `tts_model.inference(text, speech=, spembs=, use_teacher_forcing=False, alpha=)` in get_tts_audio and
get_baseline1/2/3 (espnet2/bin/sedit_inference.py:129-260; espnet2/tts/espnet_model.py:223-308;
espnet2/tts/fastspeech2/fastspeech2.py:614-782).  a3t_amd/duration.py builds such a checkpoint up to the duration
predictor; this module adds what follows it:
  - the pitch and energy predictors (VariancePredictor: the duration predictor's conv / ReLU / LayerNorm stack and
    Linear(C -> 1), on a3t_gemm, the ragged LayerNorm and a3t_duration_head, whose frames output is not used here);
  - their embeddings, Conv1d(1 -> d), added to the encoder output (a3t_fs2_variance_embed);
  - the length regulator (a3t_length_offsets, a3t_length_expand, which also applies the decoder entry's x * sqrt(d));
  - the decoder's Conformer blocks on ConformerStack.block_fwd, after_norm, feat_out;
  - the postnet (k-tap convs without bias, BatchNorm1d in eval mode folded in fp64 into the conv weights and a shift at
    load, tanh in the GEMM's epilogue; the last layer without tanh);
  - feat_gen = before + postnet(before) and, for a checkpoint with normalize: global_mvn, feat_gen_denorm (a3t_fs2_finish).
fp32 compute, eval mode, forward only.  One phone list runs at its exact lengths (tokens, then frames) on the plain kernels;
several lists run as ragged batches whose rows are computed as if alone.  A GST model takes the prompt's log-mel NORMALISED by
the checkpoint's GlobalMVN (espnet_model.py:255-262), unlike duration_predict, which feeds the raw one."""
import dataclasses
import math
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from . import ops
from ._lib import ACT_NONE, ACT_RELU, ACT_TANH, F32
from .conformer import ConformerStack
from .duration import FS2DurationConfig, FS2DurationModel
from .duration import buffer_layout as _dur_buffer_layout
from .duration import key_map as _dur_key_map
from .duration import load_into as _dur_load_into
from .duration import param_layout as _dur_param_layout
from .params import ParamStore, _block_layout, _ref_block_map
from .schedule import _RowWorkspace

# FastSpeech2.__init__ defaults of the keys the synthesis path reads beyond duration.py's
_TTS_DEFAULTS = dict(dlayers=6, dunits=1536, postnet_layers=5, postnet_chans=512, postnet_filts=5, use_batch_norm=True,
                     decoder_normalize_before=True, decoder_concat_after=False, reduction_factor=1, decoder_type="transformer",
                     conformer_dec_kernel_size=31, energy_predictor_layers=2, energy_predictor_chans=384,
                     energy_predictor_kernel_size=3, energy_embed_kernel_size=9, pitch_predictor_layers=2,
                     pitch_predictor_chans=384, pitch_predictor_kernel_size=3, pitch_embed_kernel_size=9, spks=None, langs=None)
VAR_MAX_CHANS, EMBED_MAX_KERNEL = 512, 9       # csrc/duration.hip: DUR_MAXV * 64; csrc/fs2_tts.hip: FS2_MAXK


@dataclass
class FS2TTSConfig(FS2DurationConfig):
    """FS2DurationConfig plus the decoder (dec_blocks = dlayers, dec_ff = dunits, dec_kernel), the variance predictors and
    embeddings, the postnet, odim and the feature normaliser."""
    dec_ff: int = 1536
    pitch_layers: int = 2
    pitch_chans: int = 384
    pitch_kernel: int = 3
    pitch_embed_kernel: int = 9
    energy_layers: int = 2
    energy_chans: int = 384
    energy_kernel: int = 3
    energy_embed_kernel: int = 9
    normalize: bool = False
    stats_file: Optional[str] = None
    norm_means: bool = True
    norm_vars: bool = True
    norm_eps: float = 1e-20

    @staticmethod
    def from_espnet(conf: Dict[str, Any], gst: bool = False) -> "FS2TTSConfig":
        """Translate an ESPnet TTS config.yaml (tts_conf, token_list, odim, normalize / normalize_conf, feats_extract_conf)."""
        base = FS2DurationConfig.from_espnet(conf, gst=gst)
        t = dict(_TTS_DEFAULTS)
        t.update(conf.get("tts_conf") or {})
        if t["decoder_type"] != "conformer":
            raise NotImplementedError(f"decoder_type: {t['decoder_type']!r}: only the conformer decoder is implemented")
        if int(t["reduction_factor"]) != 1:
            raise NotImplementedError(f"reduction_factor: {t['reduction_factor']!r}: only 1 is implemented")
        for name in ("spks", "langs"):
            if t[name] is not None and int(t[name]) > 1:
                raise NotImplementedError(f"{name}: {t[name]!r}: speaker / language id embeddings are not implemented")
        for name, ok in (("decoder_normalize_before", bool(t["decoder_normalize_before"])),
                         ("decoder_concat_after", not t["decoder_concat_after"])):
            if not ok:
                raise NotImplementedError(f"{name}: {t[name]!r} is not implemented")
        for name in ("pitch_predictor_kernel_size", "energy_predictor_kernel_size", "pitch_embed_kernel_size",
                     "energy_embed_kernel_size", "postnet_filts", "conformer_dec_kernel_size"):
            if int(t[name]) < 1 or int(t[name]) % 2 == 0:
                raise NotImplementedError(f"{name}: {t[name]!r}: only odd kernel sizes are implemented")
        for name in ("pitch_embed_kernel_size", "energy_embed_kernel_size"):
            if int(t[name]) > EMBED_MAX_KERNEL:
                raise NotImplementedError(f"{name}: {t[name]!r}: kernel sizes up to {EMBED_MAX_KERNEL} are implemented")
        for name in ("pitch_predictor_chans", "energy_predictor_chans"):
            if not 1 <= int(t[name]) <= VAR_MAX_CHANS:
                raise NotImplementedError(f"{name}: {t[name]!r}: 1..{VAR_MAX_CHANS} are implemented")
        for name in ("pitch_predictor_layers", "energy_predictor_layers", "dlayers"):
            if int(t[name]) < 1:
                raise ValueError(f"{name}: {t[name]!r}")
        if int(t["postnet_layers"]) > 0 and not t["use_batch_norm"]:
            raise NotImplementedError("use_batch_norm: False (a postnet without BatchNorm) is not implemented")
        if base.adim % 4:
            raise NotImplementedError(f"adim: {base.adim!r}: a multiple of 4 is implemented")
        norm = conf.get("normalize")
        nc = dict(conf.get("normalize_conf") or {})
        if norm not in (None, "global_mvn"):
            raise NotImplementedError(f"normalize: {norm!r}: only global_mvn (or none) is implemented")
        if norm is not None and not nc.get("stats_file"):
            raise ValueError("normalize: global_mvn needs normalize_conf.stats_file")
        odim = int(conf.get("odim") or (conf.get("feats_extract_conf") or {}).get("n_mels") or base.n_mels)
        kw = {f.name: getattr(base, f.name) for f in dataclasses.fields(base)}
        kw.update(odim=odim, dec_blocks=int(t["dlayers"]), dec_ff=int(t["dunits"]), dec_kernel=int(t["conformer_dec_kernel_size"]),
                  postnet_layers=int(t["postnet_layers"]), postnet_chans=int(t["postnet_chans"]),
                  postnet_filts=int(t["postnet_filts"]), pitch_layers=int(t["pitch_predictor_layers"]),
                  pitch_chans=int(t["pitch_predictor_chans"]), pitch_kernel=int(t["pitch_predictor_kernel_size"]),
                  pitch_embed_kernel=int(t["pitch_embed_kernel_size"]), energy_layers=int(t["energy_predictor_layers"]),
                  energy_chans=int(t["energy_predictor_chans"]), energy_kernel=int(t["energy_predictor_kernel_size"]),
                  energy_embed_kernel=int(t["energy_embed_kernel_size"]), normalize=norm is not None,
                  stats_file=nc.get("stats_file"), norm_means=bool(nc.get("norm_means", True)),
                  norm_vars=bool(nc.get("norm_vars", True)), norm_eps=float(nc.get("eps", 1e-20)))
        return FS2TTSConfig(**kw)

    def decoder_config(self) -> "FS2TTSConfig":
        """The config the decoder's engine reads: its feed-forward width is dunits."""
        return dataclasses.replace(self, ff=self.dec_ff)

    def variance(self, which):
        """(layers, chans, kernel, embed kernel) of "pitch" or "energy"."""
        return tuple(getattr(self, f"{which}_{n}") for n in ("layers", "chans", "kernel", "embed_kernel"))

    def postnet_dims(self):
        """(in, out) channels of every postnet layer."""
        n = self.postnet_layers
        return [(self.odim if l == 0 else self.postnet_chans, self.odim if l == n - 1 else self.postnet_chans)
                for l in range(n)]


_VAR = (("pitch", "pp", "pemb"), ("energy", "ep", "eemb"))      # (reference name, predictor prefix, embedding prefix)


def param_layout(c: FS2TTSConfig):
    d = c.adim
    lay = _dur_param_layout(c)
    for i in range(c.dec_blocks):
        for n, s in _block_layout(c.decoder_config(), c.dec_kernel):
            lay[f"dec.{i}.{n}"] = s
    lay["dec.after.g"] = (d,)
    lay["dec.after.b"] = (d,)
    for which, pre, emb in _VAR:
        layers, chans, k, ke = c.variance(which)
        for l in range(layers):
            lay[f"{pre}.{l}.w"] = (chans, k, d if l == 0 else chans)
            lay[f"{pre}.{l}.b"] = (chans,)
            lay[f"{pre}.{l}.ln.g"] = (chans,)
            lay[f"{pre}.{l}.ln.b"] = (chans,)
        lay[f"{pre}.lin.w"] = (chans,)
        lay[f"{pre}.lin.b"] = (1,)
        lay[f"{emb}.w"] = (ke, d)          # Conv1d(1 -> d, ke) weight [d][1][ke], taps outermost
        lay[f"{emb}.b"] = (d,)
    lay["fout.w"] = (c.odim, d)
    lay["fout.b"] = (c.odim,)
    for l, (ic, oc) in enumerate(c.postnet_dims()):
        lay[f"post.{l}.w"] = (oc, c.postnet_filts, ic)
        lay[f"post.{l}.bn.g"] = (oc,)
        lay[f"post.{l}.bn.b"] = (oc,)
    return lay


def buffer_layout(c: FS2TTSConfig):
    lay = _dur_buffer_layout(c)
    for i in range(c.dec_blocks):
        lay[f"dec.{i}.cnv.bn.rm"] = (c.adim,)
        lay[f"dec.{i}.cnv.bn.rv"] = (c.adim,)
    for l, (_, oc) in enumerate(c.postnet_dims()):
        lay[f"post.{l}.bn.rm"] = (oc,)
        lay[f"post.{l}.bn.rv"] = (oc,)
    return lay


def tts_key_map(c: FS2TTSConfig):
    """The entries behind duration.key_map: (checkpoint key, store name, slice | None, kind); kind "embed": a Conv1d(1 -> d, k)
    weight [d][1][k] -> [k][d]."""
    m = []
    for i in range(c.dec_blocks):
        m += _ref_block_map(f"tts.decoder.encoders.{i}.", f"dec.{i}.", c)
    m += [("tts.decoder.after_norm.weight", "dec.after.g", None, "reshape"),
          ("tts.decoder.after_norm.bias", "dec.after.b", None, "reshape")]
    for which, pre, emb in _VAR:
        for l in range(c.variance(which)[0]):
            p = f"tts.{which}_predictor.conv.{l}."
            m += [(p + "0.weight", f"{pre}.{l}.w", None, "conv"), (p + "0.bias", f"{pre}.{l}.b", None, "reshape"),
                  (p + "2.weight", f"{pre}.{l}.ln.g", None, "reshape"), (p + "2.bias", f"{pre}.{l}.ln.b", None, "reshape")]
        m += [(f"tts.{which}_predictor.linear.weight", f"{pre}.lin.w", None, "reshape"),
              (f"tts.{which}_predictor.linear.bias", f"{pre}.lin.b", None, "reshape"),
              (f"tts.{which}_embed.0.weight", f"{emb}.w", None, "embed"), (f"tts.{which}_embed.0.bias", f"{emb}.b", None, "reshape")]
    m += [("tts.feat_out.weight", "fout.w", None, "reshape"), ("tts.feat_out.bias", "fout.b", None, "reshape")]
    for l in range(c.postnet_layers):
        p = f"tts.postnet.postnet.{l}."
        m += [(p + "0.weight", f"post.{l}.w", None, "conv"), (p + "1.weight", f"post.{l}.bn.g", None, "reshape"),
              (p + "1.bias", f"post.{l}.bn.b", None, "reshape"), (p + "1.running_mean", f"post.{l}.bn.rm", None, "buffer"),
              (p + "1.running_var", f"post.{l}.bn.rv", None, "buffer")]
    return m


def key_map(c: FS2TTSConfig):
    return _dur_key_map(c) + tts_key_map(c)


_TTS_PREFIXES = ("tts.decoder.", "tts.pitch_predictor.", "tts.energy_predictor.", "tts.pitch_embed.", "tts.energy_embed.",
                 "tts.feat_out.", "tts.postnet.")


def load_into(store: ParamStore, c: FS2TTSConfig, sd) -> None:
    """duration.load_into for the text side, then the synthesis entries; a missing key, or an unknown key under the decoder,
    the variance predictors / embeddings, feat_out or the postnet (BatchNorm's num_batches_tracked aside), is an error."""
    _dur_load_into(store, c, sd)
    km = tts_key_map(c)
    missing = sorted({k for k, _, _, kind in km if k not in sd and kind != "nbt"})
    if missing:
        raise KeyError(f"FastSpeech2 checkpoint: missing keys {missing}")
    used = {k for k, _, _, _ in km}
    unexpected = sorted(k for k in set(sd) - used if k.startswith(_TTS_PREFIXES) and not k.endswith(".num_batches_tracked"))
    if unexpected:
        raise KeyError(f"FastSpeech2 checkpoint: unexpected keys {unexpected}")
    for key, name, sl, kind in km:
        if kind == "nbt":
            continue
        src = sd[key]
        if not torch.is_tensor(src):
            src = torch.as_tensor(np.asarray(src))
        dst = store.buf[name] if kind == "buffer" else store.p[name]
        if kind == "rows":
            dst = dst[sl[0]:sl[1]]
        elif kind == "conv":
            src = src.permute(0, 2, 1)
        elif kind == "embed":
            src = src[:, 0, :].t()
        dst.copy_(src.reshape(dst.shape).to(device=store.device, dtype=torch.float32))


def global_mvn_stats(stats_file, norm_means=True, norm_vars=True, eps=1e-20):
    """(mean, std) of an ESPnet feats_stats.npz as GlobalMVN.__init__ takes them (espnet2/layers/global_mvn.py:41-57), float64;
    None where the flag is off."""
    stats = np.load(stats_file)
    count = stats["count"]
    mean = stats["sum"] / count
    var = stats["sum_square"] / count - mean * mean
    std = np.sqrt(np.maximum(var, eps))
    return (mean if norm_means else None), (std if norm_vars else None)


class FS2TTSModel(FS2DurationModel):
    """Text to mel with a conformer FastSpeech2 checkpoint on one device (fp32, eval mode).  Everything of FS2DurationModel
    works as there (the same weights give the same durations)."""

    def __init__(self, cfg: FS2TTSConfig, device="cuda"):
        # FS2DurationModel.__init__ with this module's layouts: the parent would build its own, smaller store
        self.c = cfg
        self.store = ParamStore(cfg, device, layout=param_layout(cfg), buffers=buffer_layout(cfg), keymap=key_map(cfg))
        self.dev = self.store.device
        self.eng = ConformerStack(cfg, self.store, compute="f32", training=False)
        self.eng.ws = self.ws = _RowWorkspace(self.dev)
        self.eng_dec = ConformerStack(cfg.decoder_config(), self.store, compute="f32", training=False)
        self.eng_dec.ws = self.ws
        self.token2id = {}
        for i, t in enumerate(cfg.token_list):
            self.token2id.setdefault(t, i)
        if "<unk>" not in self.token2id:
            raise ValueError("token_list has no <unk>")
        self.unk_id = self.token2id["<unk>"]
        self.eos = cfg.vocab - 1
        self._seg0 = torch.zeros(1, cfg.adim, dtype=torch.float32, device=self.dev)
        self._tpos0 = torch.zeros(cfg.max_len, dtype=torch.int64, device=self.dev)
        self._keys1 = torch.ones(cfg.max_len, dtype=torch.uint8, device=self.dev)
        pin = self.dev.type == "cuda"
        self._ids_host = torch.zeros(cfg.max_len, dtype=torch.int64, pin_memory=pin)
        self._ids_dev = torch.zeros(cfg.max_len, dtype=torch.int64, device=self.dev)
        self._stage_host = self._stage_dev = None
        self.feats = None
        self._gst = None
        self._gst_lens = None
        self._tts = None        # what the synthesis path derives from the weights alone (see _tts_derived)
        self.mean = self.std = None
        if cfg.use_gst:
            from .features import LogMelFbank
            self.feats = LogMelFbank(**cfg.gst_feats_conf, device=self.dev)
        if cfg.normalize:
            self.set_global_mvn(*global_mvn_stats(cfg.stats_file, cfg.norm_means, cfg.norm_vars, cfg.norm_eps))

    # ---- loading ---------------------------------------------------------------------------------------------------------
    def set_global_mvn(self, mean, std):
        """mean, std: float64 arrays [odim] (or None: that step of GlobalMVN is off)."""
        dev = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.float64)).to(self.dev, torch.float32).contiguous()
        self.mean, self.std = dev(mean), dev(std)
        for a in (self.mean, self.std):
            if a is not None and a.numel() != self.c.odim:
                raise ValueError(f"GlobalMVN statistics of {a.numel()} values for odim {self.c.odim}")

    def load_state_dict(self, sd):
        load_into(self.store, self.c, sd)
        self._gst = self._tts = None
        return self

    @staticmethod
    def from_file(config_file: Optional[str], model_file: str, device="cuda", gst: bool = False) -> "FS2TTSModel":
        """As FS2DurationModel.from_file; a relative normalize_conf.stats_file that does not exist as given is looked for next
        to the config file."""
        import yaml
        if config_file is None:
            config_file = os.path.join(os.path.dirname(os.path.abspath(model_file)), "config.yaml")
        with open(config_file) as f:
            conf = yaml.safe_load(f)
        sf = (conf.get("normalize_conf") or {}).get("stats_file")
        if sf and not os.path.exists(sf):
            conf["normalize_conf"] = dict(conf["normalize_conf"],
                                          stats_file=os.path.join(os.path.dirname(os.path.abspath(config_file)), sf))
        model = FS2TTSModel(FS2TTSConfig.from_espnet(conf, gst=gst), device)
        return model.load_state_dict(torch.load(model_file, map_location="cpu"))

    def _tts_derived(self):
        """Once per load: every postnet layer's BatchNorm1d (running statistics, eps 1e-5) folded in fp64 into the conv
        weights, w * gamma / sqrt(var + eps) per output channel, and the shift beta - mean * gamma / sqrt(var + eps), which
        the GEMM adds as its bias."""
        if self._tts is None:
            p, buf, out = self.store.p, self.store.buf, {}
            for l in range(self.c.postnet_layers):
                n = f"post.{l}.bn."
                sc = p[n + "g"].double() / torch.sqrt(buf[n + "rv"].double() + 1e-5)
                out[f"w.{l}"] = (p[f"post.{l}.w"].double() * sc[:, None, None]).float().contiguous()
                out[f"shift.{l}"] = (p[n + "b"].double() - buf[n + "rm"].double() * sc).float().contiguous()
            self._tts = out
        return self._tts

    # ---- the prompt of a GST model ---------------------------------------------------------------------------------------
    def _norm_mel(self, mel, out=None):
        """GlobalMVN on log-mel rows [..][n_mels] (device fp32): (mel - mean) / std, or mel itself without a normaliser."""
        if self.mean is None and self.std is None:
            if out is not None:
                out.copy_(mel)
            return mel
        y = torch.empty_like(mel) if out is None else out
        ops.fs2_mvn(mel, self.mean, self.std, y)
        return y

    def style_from_prompts(self, prompts=None, prompt_mels=None):
        """Style embeddings [S][d] of prompt waveforms (1-D, at the extractor's sampling rate), or of raw log-mels [F][n_mels]
        (prompt_mels), normalised as inference does; several in one ragged pass."""
        if not self.c.use_gst:
            raise ValueError("this checkpoint has no GST style encoder")
        if (prompts is None) == (prompt_mels is None):
            raise ValueError("give prompts or prompt_mels")
        if prompts is not None:
            mels = [self._prompt_mel(w)[0][0] for w in prompts]
        else:
            mels = [torch.as_tensor(np.asarray(m, np.float32) if not torch.is_tensor(m) else m).to(self.dev, torch.float32)
                    for m in prompt_mels]
        if not mels:
            raise ValueError("no prompts")
        frames = [int(m.shape[0]) for m in mels]
        if len(mels) == 1:
            return self.style_from_mel(self._norm_mel(mels[0].contiguous())[None])
        x = self.ws.get("gst.mel", (len(mels), max(frames), self.c.n_mels))
        for b, m in enumerate(mels):
            self._norm_mel(m.contiguous(), out=x[b, :frames[b]])
        return self.style_from_mel(x, self._gst_len_table(frames))

    # ---- synthesis -------------------------------------------------------------------------------------------------------
    def _variance(self, pre, which, hs, out, T, tail):
        """One VariancePredictor over hs [M][d] (zeros behind every row's length when tail is given): out [M]."""
        c, p, ws, eng = self.c, self.store.p, self.ws, self.eng
        layers, chans, k, _ = c.variance(which)
        y, pad, M = hs, (k - 1) // 2, hs.shape[0]
        tail = tail if pad > 0 else None
        for l in range(layers):
            z = ws.get(f"{pre}.{l}.z", (M, chans))
            ops.conv_fwd(y, p[f"{pre}.{l}.w"], z, T, pad, bias=p[f"{pre}.{l}.b"], act=ACT_RELU, compute=F32)
            if l < layers - 1:
                y = eng._ln_fwd(f"{pre}.{l}.ln", z, f"{pre}.{l}.ln", out_dtype=torch.float32, lens=tail, T=T)
        l = layers - 1
        ops.duration_head(z, p[f"{pre}.{l}.ln.g"], p[f"{pre}.{l}.ln.b"], p[f"{pre}.lin.w"], p[f"{pre}.lin.b"], out,
                          ws.get("tts.unused", (M,), torch.int64), eps=1e-12, offset=0.0)

    def _text_side(self, ids, B, T, lens, spk_bias, style, style_rows, pitch, energy, frames_out, offsets, frame_lens, alpha,
                   spk_rows=None):
        """Encoder to length offsets of one chunk.  Returns hs [B*T][d] with the embeddings added (a workspace view)."""
        c, p = self.c, self.store.p
        hs, _, frames = self._forward(ids, B, T, lens, spk_bias, style, style_rows, spk_rows)
        tail = None
        if lens is not None:
            tail = lens
            if c.dp_kernel == 1 and max(c.pitch_kernel, c.energy_kernel) > 1:     # (_forward zeroes the tails otherwise)
                ops.zero_tail(hs, lens, 1, B, T)
        self._variance("pp", "pitch", hs, pitch, T, tail)
        self._variance("ep", "energy", hs, energy, T, tail)
        ops.fs2_variance_embed(hs, pitch, energy, p["pemb.w"], p["pemb.b"], p["eemb.w"], p["eemb.b"], lens, B, T)
        frames_out.copy_(frames)
        ops.length_offsets(frames.view(B, T), lens, alpha, offsets, frame_lens)
        return hs

    def _decode(self, hs, offsets, lens, frame_lens, B, T, Fp, ragged):
        """Length regulator to feat_gen for B rows of hs [B][T][d] padded to Fp frames (ragged False: B = 1 at its exact
        length).  Returns fresh tensors (before, feat_gen, feat_gen_denorm | None), each [B][Fp][odim]."""
        c, p, ws, eng = self.c, self.store.p, self.ws, self.eng_dec
        d, M = c.adim, B * Fp
        x = ws.get("tts.reg", (M, d))
        ops.length_expand(hs, offsets, lens, frame_lens, x.view(B, Fp, d), math.sqrt(d))
        flens = frame_lens if ragged else None
        keymask = None if ragged else self._keys1[:Fp].view(1, Fp)
        pos = eng.pe[:Fp]
        for i in range(c.dec_blocks):
            x = eng.block_fwd(f"dec.{i}", x, pos, keymask, B, Fp, lens=flens)
        z = eng._ln_fwd("dec.after", x, "dec.after", out_dtype=torch.float32)
        before = torch.empty(B, Fp, c.odim, dtype=torch.float32, device=self.dev)
        ops.linear_fwd(z, p["fout.w"], before.view(M, c.odim), bias=p["fout.b"], compute=F32)
        post, pad, der = None, (c.postnet_filts - 1) // 2, self._tts_derived()
        if c.postnet_layers > 0:
            y = before.view(M, c.odim)
            if ragged and pad > 0:
                ops.zero_tail(y, flens, 1, B, Fp)
            for l, (_, oc) in enumerate(c.postnet_dims()):
                last = l == c.postnet_layers - 1
                post = ws.get(f"tts.post.{l % 2}", (M, oc))
                ops.conv_fwd(y, der[f"w.{l}"], post, Fp, pad, bias=der[f"shift.{l}"], act=ACT_NONE if last else ACT_TANH,
                             compute=F32)
                if ragged and pad > 0 and not last:      # the shift and tanh make the tail non-zero; the next taps read 0 there
                    ops.zero_tail(post, flens, 1, B, Fp)
                y = post
            post = post.view(B, Fp, c.odim)
        after = torch.empty_like(before)
        denorm = torch.empty_like(before) if (self.mean is not None or self.std is not None) else None
        ops.fs2_finish(before, post, after, lens=flens, mean=self.mean, std=self.std, denorm=denorm)
        return before, after, denorm

    def synthesize_ids_batch(self, id_lists, spembs=None, style=None, style_rows=None, alpha: float = 1.0,
                             max_score_elems: int = 1 << 24, speakers=None) -> List[Dict[str, torch.Tensor]]:
        """The body of synthesize_batch on token ids (eos included): one dict of device tensors per list.
        style (a GST model): [len(id_lists)][d], [1][d], or [S][d] with style_rows (a host list), as predict_frames_batch.
        speakers (instead of spembs): one x-vector per list; see synthesize_batch."""
        c = self.c
        lists = [[int(i) for i in ids] for ids in id_lists]
        if not lists:
            return []
        if not (float(alpha) > 0.0):
            raise ValueError(f"alpha {alpha!r} must be positive")
        if spembs is not None and speakers is not None:
            raise ValueError("give spembs (one x-vector for all lists) or speakers (one per list), not both")
        n = len(lists)
        krow = None
        if speakers is not None:
            speakers = list(speakers)
            if len(speakers) != n:
                raise ValueError(f"speakers: {len(speakers)} x-vectors for {n} phone lists")
            for i, x in enumerate(speakers):
                if x is None:
                    raise ValueError(f"speakers[{i}] is None: synthesis needs an x-vector for every list")
            bias, krow = self.speaker_bias_table(speakers)
        else:
            if spembs is None and c.spk_embed_dim > 0:
                raise ValueError("this checkpoint needs spembs (its x-vector projection is part of inference)")
            bias = self.speaker_bias(spembs) if spembs is not None else None
        srow = None
        self._check_style(style, n, style_rows)
        if style is not None:
            srow = [0] * n if style_rows is None and style.shape[0] == 1 else \
                list(range(n)) if style_rows is None else [int(r) for r in style_rows]
            if len(srow) != n or min(srow) < 0 or max(srow) >= style.shape[0]:
                raise ValueError("style_rows does not fit the lists and the style rows")
        lengths = [len(x) for x in lists]
        if min(lengths) < 1 or max(lengths) > c.max_len:
            raise ValueError(f"token counts {min(lengths)}..{max(lengths)} outside 1..{c.max_len}")
        chunks = self._chunks(lengths, int(max_score_elems))
        # staging (int64 words): per chunk its padded ids [B][Tmax]; then the lengths and the style rows as int32 (with
        # speakers: their table rows as int32 behind those)
        offs, n_ids = [], 0
        for ch in chunks:
            offs.append(n_ids)
            n_ids += len(ch) * lengths[ch[-1]]
        total = n_ids + n + (0 if krow is None else (n + 1) // 2)
        if self._stage_host is None or self._stage_host.numel() < total:
            cap = max(total, 2 * (self._stage_host.numel() if self._stage_host is not None else 0))
            self._stage_host = torch.zeros(cap, dtype=torch.int64, pin_memory=self.dev.type == "cuda")
            self._stage_dev = torch.zeros(cap, dtype=torch.int64, device=self.dev)
        host = np.zeros(total, np.int64)
        hl = host[n_ids:].view(np.int32)
        r = 0
        for ch, o in zip(chunks, offs):
            T = lengths[ch[-1]]
            blk = host[o:o + len(ch) * T].reshape(len(ch), T)
            for k, i in enumerate(ch):
                blk[k, :lengths[i]] = lists[i]
                hl[r + k] = lengths[i]
                hl[n + r + k] = 0 if srow is None else srow[i]
                if krow is not None:
                    hl[2 * n + r + k] = krow[i]
            r += len(ch)
        # the pinned staging buffer is free again: the previous call's copy finished before its result reached the host
        self._stage_host[:total].copy_(torch.from_numpy(host))
        dev = self._stage_dev[:total]
        dev.copy_(self._stage_host[:total], non_blocking=True)
        dev_lens = dev[n_ids:].view(torch.int32)
        # per call: what comes back to the host in one copy (the durations, then the frame counts as int32), and the outputs
        down = torch.empty(n_ids + (n + 1) // 2, dtype=torch.int64, device=self.dev)
        flens_dev = down[n_ids:].view(torch.int32)
        pitch = torch.empty(n_ids, dtype=torch.float32, device=self.dev)
        energy = torch.empty(n_ids, dtype=torch.float32, device=self.dev)
        offsets = torch.empty(n_ids + n, dtype=torch.int32, device=self.dev)
        hs_all = torch.empty(n_ids, c.adim, dtype=torch.float32, device=self.dev) if len(chunks) > 1 else None
        r, hs_one = 0, None
        for ch, o in zip(chunks, offs):
            B, T = len(ch), lengths[ch[-1]]
            sl = slice(o, o + B * T)
            off = offsets[o + r:o + r + B * (T + 1)].view(B, T + 1)
            if B == 1:      # (with speakers: this list's own table row is the one bias of the B = 1 path)
                hs = self._text_side(dev[sl], 1, T, None, bias if krow is None else bias[krow[ch[0]]:krow[ch[0]] + 1],
                                     None if style is None else style[srow[ch[0]]:srow[ch[0]] + 1],
                                     None, pitch[sl], energy[sl], down[sl], off, flens_dev[r:r + 1], alpha)
            else:
                rows = None if style is None else dev_lens[n + r:n + r + B]
                krows = None if krow is None else dev_lens[2 * n + r:2 * n + r + B]
                hs = self._text_side(dev[sl].view(B, T), B, T, dev_lens[r:r + B], bias, style, rows, pitch[sl], energy[sl],
                                     down[sl], off, flens_dev[r:r + B], alpha, krows)
            if hs_all is None:
                hs_one = hs
            else:
                hs_all[sl].copy_(hs)
            r += B
        got = down.cpu().numpy()        # the call's one copy to the host: it sizes the decoder's workspace
        fl = got[n_ids:].view(np.int32)
        res: List[Optional[Dict[str, torch.Tensor]]] = [None] * n
        r = 0
        for ch, o in zip(chunks, offs):
            B, T = len(ch), lengths[ch[-1]]
            F_rows = [int(fl[r + k]) for k in range(B)]
            for k, i in enumerate(ch):
                if F_rows[k] < 1:
                    raise ValueError(f"phone list {i}: its durations sum to 0 frames, nothing to decode")
                if F_rows[k] > c.max_len:
                    raise ValueError(f"phone list {i}: {F_rows[k]} frames: more than max_len {c.max_len}")
            hs3 = (hs_one if hs_all is None else hs_all[o:o + B * T]).view(B, T, c.adim)
            off = offsets[o + r:o + r + B * (T + 1)].view(B, T + 1)
            # rows of the chunk in order, cut where B * H * Fmax^2 would pass the cap (a row too long for it runs alone)
            k0 = 0
            while k0 < B:
                k1, Fp = k0 + 1, F_rows[k0]
                while k1 < B and (k1 + 1 - k0) * c.heads * max(Fp, F_rows[k1]) ** 2 <= int(max_score_elems):
                    Fp = max(Fp, F_rows[k1])
                    k1 += 1
                nb = k1 - k0
                before, after, denorm = self._decode(hs3[k0:k1], off[k0:k1], None if B == 1 else dev_lens[r + k0:r + k1],
                                                     flens_dev[r + k0:r + k1], nb, T, Fp, ragged=nb > 1)
                for k in range(k0, k1):
                    i, Fk, s = ch[k], F_rows[k], slice(o + k * T, o + k * T + lengths[ch[k]])
                    out = dict(feat_gen=after[k - k0, :Fk], before=before[k - k0, :Fk], duration=down[s], pitch=pitch[s],
                               energy=energy[s])
                    if denorm is not None:
                        out["feat_gen_denorm"] = denorm[k - k0, :Fk]
                    res[i] = out
                k0 = k1
            r += B
        return res

    def _styles(self, n, prompts, prompt_mels):
        """(style, style_rows) of one prompt per list (a list) or one prompt for all (a single waveform / mel); one style row per
        distinct prompt OBJECT."""
        if not self.c.use_gst:
            if prompts is not None or prompt_mels is not None:
                raise ValueError("prompt given but the checkpoint has no GST style encoder")
            return None, None
        if (prompts is None) == (prompt_mels is None):
            raise ValueError("a GST model needs the prompt (prompts= waveforms, or prompt_mels= raw log-mels) with every call")
        given = prompts if prompts is not None else prompt_mels
        if not isinstance(given, (list, tuple)):
            given = [given] * n
        if len(given) != n:
            raise ValueError(f"{len(given)} prompts for {n} phone lists")
        first = {}
        rows = [first.setdefault(id(w), len(first)) for w in given]
        distinct = [None] * len(first)
        for w, r in zip(given, rows):
            distinct[r] = w
        style = self.style_from_prompts(distinct) if prompts is not None else self.style_from_prompts(prompt_mels=distinct)
        return style, rows

    def synthesize_batch(self, lists, spembs=None, prompts=None, alpha: float = 1.0, prompt_mels=None,
                         max_score_elems: int = 1 << 24, speakers=None) -> List[Dict[str, torch.Tensor]]:
        """ESPnetTTSModel.inference(text, speech=prompt, spembs=, use_teacher_forcing=False, alpha=) for several phone lists:
        one dict per list, in the order given, of device tensors feat_gen [F][odim], feat_gen_denorm (a normalising checkpoint
        only), duration [T] int64 (eos entry included; as the reference, not scaled by alpha), pitch [T], energy [T], and
        `before` [F][odim] (the mel in front of the postnet).
        The lists are sorted by length and cut into chunks as predict_frames_batch cuts them; max_score_elems caps
        B * H * Tmax^2 of a chunk and B * H * Fmax^2 of its decoder pass (a chunk whose frames pass the cap is decoded in
        parts).  Every row is computed as if alone.  One copy to the host per call -- the durations and frame counts, which
        size the decoder's buffers; the number of launches of a chunk does not depend on its rows.
        prompts (a GST model): one waveform per list, or one for all; prompt_mels: raw log-mels [F][n_mels] instead.
        spembs: one x-vector behind all lists; speakers: one per list instead (the same object may repeat: one speaker bias per
        distinct OBJECT, FS2DurationModel.speaker_bias_table) -- the rows follow the lists through the text-side chunks, and the
        decoder does not read the x-vector.  Giving both is an error.
        A list whose durations sum to 0 frames raises ValueError (after the copy): there is nothing to decode."""
        lists = [list(ph) for ph in lists]
        if spembs is not None and speakers is not None:
            raise ValueError("give spembs (one x-vector for all lists) or speakers (one per list), not both")
        style, rows = self._styles(len(lists), prompts, prompt_mels) if lists else (None, None)
        return self.synthesize_ids_batch([self.tokens_to_ids(ph) for ph in lists], spembs, style, rows, alpha, max_score_elems,
                                         speakers)

    def synthesize(self, phns, spembs=None, prompt=None, alpha: float = 1.0, prompt_mel=None) -> Dict[str, torch.Tensor]:
        """synthesize_batch for one phone list: at its exact lengths, on the plain kernels."""
        return self.synthesize_batch([phns], spembs, None if prompt is None else [prompt], alpha,
                                     None if prompt_mel is None else [prompt_mel])[0]
