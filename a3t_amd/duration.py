"""Conformer FastSpeech2 duration model on the device: the phone durations of the speech-editing driver.

The reference asks the user's own torch FastSpeech2 for them (espnet2/bin/sedit_inference.py:398-425 duration_predict,
twice per edit with duration_adjust).  Only the part of FastSpeech2 that duration_predict runs is built here:
  - the text encoder (espnet/nets/pytorch_backend/conformer/encoder.py with an Embedding input layer): Embedding * sqrt(d)
    (LegacyRelPositionalEncoding), the Conformer blocks of ConformerStack.block_fwd, after_norm;
  - the x-vector integration (espnet2/tts/fastspeech2/fastspeech2.py:784-808, "add" or "concat");
  - the DurationPredictor (espnet/nets/pytorch_backend/fastspeech/duration_predictor.py) in inference mode: k-tap convs
    with ReLU and LayerNorm, then a3t_duration_head (last LayerNorm, Linear(C -> 1), clamp(round(exp(x) - offset), 0)).
fp32 compute, eval mode.  A single phone sequence runs as its own B = 1 forward at its exact length n + 1 (the appended eos):
legacy rel-pos attention reads pe[:T] and the conv module does not mask padded frames, so plain padding would change the
result.  Several sequences run as ONE padded forward with per-row lengths (forward_ids_batch): the engine's ragged block
forward gives every row what it would get alone -- rel_shift at the row's own length, zeros behind it for every k-tap conv.

A gst+xvector checkpoint (use_gst: true; the reference's VCTK and LibriTTS duration models) is loaded with gst=True: its
durations depend on the prompt.  duration_predict (:413-418) takes the log-mel of the original waveform with the TTS model's own
extractor, runs the StyleEncoder over it (espnet2/tts/gst/style_encoder.py: stride-2 Conv2d + BatchNorm2d + ReLU layers, a
GRU, multi-head attention over learned style tokens) and adds the style embedding to every encoder output row in front of the
x-vector integration.  Here that is style_embedding(_batch) (csrc/gst.hip: one launch per conv layer, one GEMM for the GRU's
input projections, one launch for the recurrence and the token attention, whatever the number of prompts) and the style=
argument of the forwards.
"""
import math
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from . import ops
from ._lib import ACT_NONE, ACT_RELU, F32
from .config import A3TConfig
from .conformer import ConformerStack, score_chunks
from .params import ParamStore, _block_layout, _ref_block_map
from .schedule import _RowWorkspace

# FastSpeech2.__init__ defaults (espnet2/tts/fastspeech2/fastspeech2.py) of the keys the duration path reads
_FS2_DEFAULTS = dict(adim=384, aheads=4, elayers=6, eunits=1536, positionwise_layer_type="conv1d",
                     positionwise_conv_kernel_size=1, encoder_normalize_before=True, encoder_concat_after=False,
                     encoder_type="transformer", conformer_rel_pos_type="legacy", conformer_pos_enc_layer_type="rel_pos",
                     conformer_self_attn_layer_type="rel_selfattn", conformer_activation_type="swish",
                     use_macaron_style_in_conformer=True, use_cnn_in_conformer=True, zero_triu=False,
                     conformer_enc_kernel_size=7, duration_predictor_layers=2, duration_predictor_chans=384,
                     duration_predictor_kernel_size=3, spk_embed_dim=None, spk_embed_integration_type="add",
                     use_gst=False, gst_tokens=10, gst_heads=4, gst_conv_layers=6,
                     gst_conv_chans_list=(32, 32, 64, 64, 128, 128), gst_conv_kernel_size=3, gst_conv_stride=2, gst_gru_layers=1,
                     gst_gru_units=128)
# LogMelFbank.__init__ defaults (espnet2/tts/feats_extract/log_mel_fbank.py)
_FBANK_DEFAULTS = dict(fs=16000, n_fft=1024, win_length=None, hop_length=256, window="hann", center=True, normalized=False,
                       onesided=True, n_mels=80, fmin=80, fmax=7600, htk=False, log_base=10.0)
GST_MAX_UNITS, GST_MAX_DIM, GST_MAX_SCORES = 128, 1024, 512      # csrc/gst.hip: GST_MAXH, GST_MAXD, GST_MAXS

@dataclass
class FS2DurationConfig(A3TConfig):
    """A3TConfig's block fields (adim, heads, ff, ff_kernel, enc_blocks, enc_kernel, vocab) as FastSpeech2's adim, aheads,
    eunits, positionwise_conv_kernel_size, elayers, conformer_enc_kernel_size, len(token_list); the MLM-only parts off.
    spk_embed_dim is FastSpeech2's (0: no x-vector)."""
    dec_blocks: int = 0
    postnet_layers: int = 0
    dp_layers: int = 2
    dp_chans: int = 384
    dp_kernel: int = 3
    dp_offset: float = 1.0
    spk_integration: str = "add"
    token_list: List[str] = field(default_factory=list)
    # the GST style encoder (use_gst; token dim = adim, input = n_mels) and the TTS model's own log-mel extractor
    use_gst: bool = False
    gst_tokens: int = 10
    gst_heads: int = 4
    gst_conv_chans: List[int] = field(default_factory=lambda: [32, 32, 64, 64, 128, 128])
    gst_conv_kernel: int = 3
    gst_conv_stride: int = 2
    gst_gru_units: int = 128
    gst_feats_conf: Dict[str, Any] = field(default_factory=dict)

    def gst_plan(self):
        """Per conv layer of the reference encoder (Cin, Cout, Fin, Fout); the GRU input is Fout * Cout of the last."""
        k, s, F, cin, plan = self.gst_conv_kernel, self.gst_conv_stride, self.n_mels, 1, []
        for cout in self.gst_conv_chans:
            Fo = gst_out_len(F, k, s)
            plan.append((cin, cout, F, Fo))
            F, cin = Fo, cout
        return plan

    @staticmethod
    def from_espnet(conf: Dict[str, Any], gst: bool = False) -> "FS2DurationConfig":
        """Translate an ESPnet TTS config.yaml (tts: fastspeech2, tts_conf, token_list).  A use_gst: true config needs
        gst=True: the durations of such a model depend on a prompt waveform that every call then has to bring."""
        if conf.get("tts", "fastspeech2") != "fastspeech2":
            raise NotImplementedError(f"tts: {conf.get('tts')!r}: only fastspeech2 is implemented")
        tl = list(conf.get("token_list") or [])
        if not tl:
            raise ValueError("config has no token_list")
        t = dict(_FS2_DEFAULTS)
        t.update(conf.get("tts_conf") or {})
        if t["use_gst"] and not gst:
            raise NotImplementedError("use_gst: true (the GST style encoder) makes the durations depend on a prompt: "
                                      "load the checkpoint with gst=True and give the prompt with every call")
        if gst and not t["use_gst"]:
            raise ValueError("gst=True, but the config has use_gst: false")
        if t["encoder_type"] != "conformer":
            raise NotImplementedError(f"encoder_type: {t['encoder_type']!r}: only the conformer encoder is implemented")
        if t["conformer_rel_pos_type"] != "legacy":
            raise NotImplementedError(f"conformer_rel_pos_type: {t['conformer_rel_pos_type']!r}: only legacy is implemented")
        checks = [("conformer_pos_enc_layer_type", t["conformer_pos_enc_layer_type"] in ("rel_pos", "legacy_rel_pos")),
                  ("conformer_self_attn_layer_type",
                   t["conformer_self_attn_layer_type"] in ("rel_selfattn", "legacy_rel_selfattn")),
                  ("positionwise_layer_type", t["positionwise_layer_type"] == "conv1d"),
                  ("use_macaron_style_in_conformer", bool(t["use_macaron_style_in_conformer"])),
                  ("use_cnn_in_conformer", bool(t["use_cnn_in_conformer"])),
                  ("encoder_normalize_before", bool(t["encoder_normalize_before"])),
                  ("encoder_concat_after", not t["encoder_concat_after"]),
                  ("conformer_activation_type", t["conformer_activation_type"] == "swish"),
                  ("zero_triu", not t["zero_triu"])]
        for name, ok in checks:
            if not ok:
                raise NotImplementedError(f"{name}: {t[name]!r} is not implemented")
        spk = int(t["spk_embed_dim"] or 0)
        if spk > 0 and t["spk_embed_integration_type"] not in ("add", "concat"):
            raise NotImplementedError(f"spk_embed_integration_type: {t['spk_embed_integration_type']!r}: "
                                      "only add and concat are implemented")
        if t["positionwise_conv_kernel_size"] % 2 == 0 or t["duration_predictor_kernel_size"] % 2 == 0:
            raise NotImplementedError("even kernel sizes are not implemented")
        g = _gst_fields(conf, t) if t["use_gst"] else {}
        return FS2DurationConfig(**g, vocab=len(tl), adim=t["adim"], heads=t["aheads"], ff=t["eunits"],
                                 ff_kernel=t["positionwise_conv_kernel_size"], enc_blocks=t["elayers"],
                                 enc_kernel=t["conformer_enc_kernel_size"], dp_layers=t["duration_predictor_layers"],
                                 dp_chans=t["duration_predictor_chans"], dp_kernel=t["duration_predictor_kernel_size"],
                                 spk_embed_dim=spk, spk_integration=t["spk_embed_integration_type"], token_list=tl,
                                 dropout_rate=0.0, positional_dropout_rate=0.0, attention_dropout_rate=0.0)


def gst_out_len(n: int, k: int, s: int) -> int:
    """Output length of one conv layer of the reference encoder along either axis: padding (k - 1) // 2, stride s."""
    return (n + 2 * ((k - 1) // 2) - k) // s + 1


def _gst_fields(conf, t) -> Dict[str, Any]:
    """The GST fields of FS2DurationConfig from tts_conf (defaults merged in `t`) and feats_extract(_conf)."""
    if int(t["gst_gru_layers"]) != 1:
        raise NotImplementedError(f"gst_gru_layers: {t['gst_gru_layers']!r}: only one GRU layer is implemented")
    k, s = int(t["gst_conv_kernel_size"]), int(t["gst_conv_stride"])
    if k < 1 or k % 2 == 0:
        raise NotImplementedError(f"gst_conv_kernel_size: {k!r}: only odd kernel sizes are implemented")
    if s < 1:
        raise NotImplementedError(f"gst_conv_stride: {s!r} is not implemented")
    chans = [int(x) for x in t["gst_conv_chans_list"]]
    if int(t["gst_conv_layers"]) != len(chans) or not chans or min(chans) < 1:
        raise ValueError(f"gst_conv_layers: {t['gst_conv_layers']!r} does not fit gst_conv_chans_list {chans}")
    units, heads, tokens = int(t["gst_gru_units"]), int(t["gst_heads"]), int(t["gst_tokens"])
    if not 1 <= units <= GST_MAX_UNITS:
        raise NotImplementedError(f"gst_gru_units: {units!r}: 1..{GST_MAX_UNITS} are implemented")
    if heads < 1 or t["adim"] % heads != 0:
        raise ValueError(f"gst_heads: {heads!r} does not divide adim {t['adim']}")
    if tokens < 1 or heads * tokens > GST_MAX_SCORES:
        raise NotImplementedError(f"gst_tokens: {tokens!r}: gst_heads * gst_tokens up to {GST_MAX_SCORES} is implemented")
    if t["adim"] > GST_MAX_DIM:
        raise NotImplementedError(f"adim: {t['adim']!r}: a style token dimension up to {GST_MAX_DIM} is implemented")
    fe = conf.get("feats_extract", "fbank")
    if fe != "fbank":
        raise NotImplementedError(f"feats_extract: {fe!r}: only fbank is implemented")
    fc = dict(_FBANK_DEFAULTS)
    given = dict(conf.get("feats_extract_conf") or {})
    unknown = sorted(set(given) - set(fc))
    if unknown:
        raise NotImplementedError(f"feats_extract_conf: unknown keys {unknown}")
    fc.update(given)
    if fc["log_base"] is None or float(fc["log_base"]) != 10.0:
        raise NotImplementedError(f"log_base: {fc['log_base']!r}: only 10 is implemented")
    fc.pop("log_base")
    fc["fs"] = int(fc["fs"])        # (a config may spell it "24000"; "24k" style strings are not translated)
    return dict(use_gst=True, gst_tokens=tokens, gst_heads=heads, gst_conv_chans=chans, gst_conv_kernel=k, gst_conv_stride=s,
                gst_gru_units=units, gst_feats_conf=fc, n_mels=int(fc["n_mels"]))


def param_layout(c: FS2DurationConfig):
    d = c.adim
    lay = {"temb": (c.vocab, d)}
    for i in range(c.enc_blocks):
        for n, s in _block_layout(c, c.enc_kernel):
            lay[f"enc.{i}.{n}"] = s
    lay["enc.after.g"] = (d,)
    lay["enc.after.b"] = (d,)
    if c.spk_embed_dim > 0:
        if c.spk_integration == "concat":      # projection(cat[hs, s]) = hs W_h^T + (W_s s + b)
            lay["spk.wh"] = (d, d)
        lay["spk.ws"] = (d, c.spk_embed_dim)
        lay["spk.b"] = (d,)
    for l in range(c.dp_layers):
        lay[f"dp.{l}.w"] = (c.dp_chans, c.dp_kernel, d if l == 0 else c.dp_chans)
        lay[f"dp.{l}.b"] = (c.dp_chans,)
        lay[f"dp.{l}.ln.g"] = (c.dp_chans,)
        lay[f"dp.{l}.ln.b"] = (c.dp_chans,)
    lay["dp.lin.w"] = (c.dp_chans,)
    lay["dp.lin.b"] = (1,)
    if c.use_gst:
        k, H, dk = c.gst_conv_kernel, c.gst_gru_units, d // c.gst_heads
        plan = c.gst_plan()
        for i, (cin, cout, _, _) in enumerate(plan):
            lay[f"gst.conv.{i}.w"] = (k, k, cin, cout)          # [time tap][frequency tap][Cin][Cout]: channels-last
            lay[f"gst.conv.{i}.bn.g"] = (cout,)
            lay[f"gst.conv.{i}.bn.b"] = (cout,)
        lay["gst.gru.wih"] = (3 * H, plan[-1][3] * plan[-1][1])     # columns f * C + c: the conv output is channels-last
        lay["gst.gru.whh"] = (3 * H, H)
        lay["gst.gru.bih"] = (3 * H,)
        lay["gst.gru.bhh"] = (3 * H,)
        lay["gst.stl.embs"] = (c.gst_tokens, dk)
        for n, kin in (("q", H), ("k", dk), ("v", dk), ("out", d)):
            lay[f"gst.stl.{n}.w"] = (d, kin)
            lay[f"gst.stl.{n}.b"] = (d,)
    return lay


def buffer_layout(c: FS2DurationConfig):
    lay = {}
    for i in range(c.enc_blocks):
        lay[f"enc.{i}.cnv.bn.rm"] = (c.adim,)
        lay[f"enc.{i}.cnv.bn.rv"] = (c.adim,)
    if c.use_gst:
        for i, cout in enumerate(c.gst_conv_chans):
            lay[f"gst.conv.{i}.bn.rm"] = (cout,)
            lay[f"gst.conv.{i}.bn.rv"] = (cout,)
    return lay


def key_map(c: FS2DurationConfig):
    """(ESPnet TTS checkpoint key, store name, (column slice) | None, kind): ParamStore's kinds, plus "cols", "conv2d"
    (Conv2d weight [Cout][Cin][kt][kf] -> [kt][kf][Cin][Cout]) and "gru_ih" (weight_ih columns c * F + f -> f * C + c, (C, F))."""
    d = c.adim
    m = [("tts.encoder.embed.0.weight", "temb", None, "reshape")]
    for i in range(c.enc_blocks):
        m += _ref_block_map(f"tts.encoder.encoders.{i}.", f"enc.{i}.", c)
    m += [("tts.encoder.after_norm.weight", "enc.after.g", None, "reshape"),
          ("tts.encoder.after_norm.bias", "enc.after.b", None, "reshape")]
    if c.spk_embed_dim > 0:
        if c.spk_integration == "concat":
            m += [("tts.projection.weight", "spk.wh", (0, d), "cols"),
                  ("tts.projection.weight", "spk.ws", (d, d + c.spk_embed_dim), "cols")]
        else:
            m += [("tts.projection.weight", "spk.ws", None, "reshape")]
        m += [("tts.projection.bias", "spk.b", None, "reshape")]
    for l in range(c.dp_layers):
        p = f"tts.duration_predictor.conv.{l}."
        m += [(p + "0.weight", f"dp.{l}.w", None, "conv"), (p + "0.bias", f"dp.{l}.b", None, "reshape"),
              (p + "2.weight", f"dp.{l}.ln.g", None, "reshape"), (p + "2.bias", f"dp.{l}.ln.b", None, "reshape")]
    m += [("tts.duration_predictor.linear.weight", "dp.lin.w", None, "reshape"),
          ("tts.duration_predictor.linear.bias", "dp.lin.b", None, "reshape")]
    if c.use_gst:
        plan = c.gst_plan()
        for i in range(len(plan)):
            cv, bn = f"tts.gst.ref_enc.convs.{3 * i}.", f"tts.gst.ref_enc.convs.{3 * i + 1}."
            m += [(cv + "weight", f"gst.conv.{i}.w", None, "conv2d"),
                  (bn + "weight", f"gst.conv.{i}.bn.g", None, "reshape"), (bn + "bias", f"gst.conv.{i}.bn.b", None, "reshape"),
                  (bn + "running_mean", f"gst.conv.{i}.bn.rm", None, "buffer"),
                  (bn + "running_var", f"gst.conv.{i}.bn.rv", None, "buffer")]
        g = "tts.gst.ref_enc.gru."
        m += [(g + "weight_ih_l0", "gst.gru.wih", (plan[-1][1], plan[-1][3]), "gru_ih"),
              (g + "weight_hh_l0", "gst.gru.whh", None, "reshape"), (g + "bias_ih_l0", "gst.gru.bih", None, "reshape"),
              (g + "bias_hh_l0", "gst.gru.bhh", None, "reshape"), ("tts.gst.stl.gst_embs", "gst.stl.embs", None, "reshape")]
        for n in ("q", "k", "v", "out"):
            m += [(f"tts.gst.stl.mha.linear_{n}.weight", f"gst.stl.{n}.w", None, "reshape"),
                  (f"tts.gst.stl.mha.linear_{n}.bias", f"gst.stl.{n}.b", None, "reshape")]
    return m


def load_into(store: ParamStore, c: FS2DurationConfig, sd) -> None:
    """Copy an ESPnet TTS state dict (keys `tts.*`, `normalize.*`, ...) into the store.  Entries duration_predict never
    reads -- the decoder, the variance predictors and embeddings, the postnet, feat_out, sid_emb / lid_emb, the feature
    normalisers -- are ignored; a missing required key, or an unknown key under tts.encoder / tts.duration_predictor /
    tts.projection, is an error that lists them."""
    keys = set(sd)
    km = key_map(c)
    missing = sorted({k for k, _, _, _ in km if k not in keys})
    if missing:
        raise KeyError(f"FastSpeech2 checkpoint: missing keys {missing}")
    used = {k for k, _, _, _ in km}
    unexpected = sorted(k for k in keys - used
                        if k.startswith(("tts.encoder.", "tts.duration_predictor.", "tts.projection.", "tts.gst."))
                        and not (k.startswith("tts.gst.") and k.endswith(".num_batches_tracked")))
    if unexpected:
        raise KeyError(f"FastSpeech2 checkpoint: unexpected keys {unexpected}")
    for key, name, sl, kind in km:
        src = sd[key]
        if not torch.is_tensor(src):
            src = torch.as_tensor(np.asarray(src))
        if kind == "nbt":
            store.nbt[name] = int(src)
            continue
        dst = store.buf[name] if kind == "buffer" else store.p[name]
        if kind == "rows":
            dst = dst[sl[0]:sl[1]]
        elif kind == "cols":
            src = src[:, sl[0]:sl[1]]
        elif kind == "conv":
            src = src.permute(0, 2, 1)
        elif kind == "conv2d":
            src = src.permute(2, 3, 1, 0)
        elif kind == "gru_ih":
            src = src.reshape(src.shape[0], sl[0], sl[1]).permute(0, 2, 1)
        dst.copy_(src.reshape(dst.shape).to(device=store.device, dtype=torch.float32))


class FS2DurationModel:
    """The duration path of a conformer FastSpeech2 checkpoint on one device (fp32, eval mode)."""

    def __init__(self, cfg: FS2DurationConfig, device="cuda"):
        self.c = cfg
        self.store = ParamStore(cfg, device, layout=param_layout(cfg), buffers=buffer_layout(cfg), keymap=key_map(cfg))
        self.dev = self.store.device
        self.eng = ConformerStack(cfg, self.store, compute="f32", training=False)
        self.eng.ws = self.ws = _RowWorkspace(self.dev)
        self.token2id = {}
        for i, t in enumerate(cfg.token_list):
            self.token2id.setdefault(t, i)
        if "<unk>" not in self.token2id:
            raise ValueError("token_list has no <unk>")
        self.unk_id = self.token2id["<unk>"]
        self.eos = cfg.vocab - 1
        self._seg0 = torch.zeros(1, cfg.adim, dtype=torch.float32, device=self.dev)     # one-row zero segment table
        self._tpos0 = torch.zeros(cfg.max_len, dtype=torch.int64, device=self.dev)
        self._keys1 = torch.ones(cfg.max_len, dtype=torch.uint8, device=self.dev)       # no padded keys: B = 1, exact T
        self._ids_host = torch.zeros(cfg.max_len, dtype=torch.int64, pin_memory=self.dev.type == "cuda")
        self._ids_dev = torch.zeros(cfg.max_len, dtype=torch.int64, device=self.dev)
        self._stage_host = self._stage_dev = None       # predict_frames_batch: ids and lengths of one call, grow-only
        self.feats = None
        self._gst = None        # what the style encoder derives from the weights alone (see _gst_derived)
        self._gst_lens = None   # (pinned host, device, copy event): int32 length table of one style_embedding_batch call
        if cfg.use_gst:
            from .features import LogMelFbank
            self.feats = LogMelFbank(**cfg.gst_feats_conf, device=self.dev)

    # ---- loading ---------------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd):
        load_into(self.store, self.c, sd)
        self._gst = None
        return self

    @staticmethod
    def from_file(config_file: Optional[str], model_file: str, device="cuda", gst: bool = False) -> "FS2DurationModel":
        """As espnet2's Text2Speech(train_config, model_file): config_file=None reads config.yaml next to model_file.
        gst=True loads a use_gst: true checkpoint (FS2DurationConfig.from_espnet)."""
        import yaml
        if config_file is None:
            config_file = os.path.join(os.path.dirname(os.path.abspath(model_file)), "config.yaml")
        with open(config_file) as f:
            conf = yaml.safe_load(f)
        model = FS2DurationModel(FS2DurationConfig.from_espnet(conf, gst=gst), device)
        return model.load_state_dict(torch.load(model_file, map_location="cpu"))

    # ---- forward ---------------------------------------------------------------------------------------------------------
    def tokens_to_ids(self, phns) -> List[int]:
        """duration_predict's mapping: `sp` -> <blank>, tokens outside token_list -> <unk> (TokenIDConverter), + eos."""
        return [self.token2id.get("<blank>" if p == "sp" else p, self.unk_id) for p in phns] + [self.eos]

    def speaker_bias(self, spembs):
        """Device vector W_s normalize(spembs) + b of the x-vector integration: [1][d]."""
        c = self.c
        if c.spk_embed_dim <= 0:
            raise ValueError("this checkpoint has no x-vector projection (spk_embed_dim is 0)")
        s = torch.as_tensor(np.asarray(spembs, np.float32)).reshape(1, -1)
        if s.shape[1] != c.spk_embed_dim:
            raise ValueError(f"spembs has {s.shape[1]} values, the checkpoint expects {c.spk_embed_dim}")
        s = s.to(self.dev)
        sn = torch.empty_like(s)
        ops.l2_normalize(s, sn)
        out = torch.empty(1, c.adim, dtype=torch.float32, device=self.dev)
        ops.linear_fwd(sn, self.store.p["spk.ws"], out, bias=self.store.p["spk.b"], compute=F32)
        return out

    def speaker_bias_table(self, spembs_list):
        """speaker_bias for several x-vectors: (table [S][d] on the device, rows), rows[i] the table row of spembs_list[i].
        One row per distinct x-vector OBJECT, in first-use order (as batch(..., prompts=) finds distinct prompts); the S vectors
        go up in one copy, through one normalisation and one GEMM."""
        c = self.c
        if c.spk_embed_dim <= 0:
            raise ValueError("this checkpoint has no x-vector projection (spk_embed_dim is 0)")
        first, host = {}, []
        rows = []
        for i, x in enumerate(spembs_list):
            if id(x) not in first:
                v = np.asarray(x, np.float32).reshape(-1)
                if v.shape[0] != c.spk_embed_dim:
                    raise ValueError(f"spembs has {v.shape[0]} values, the checkpoint expects {c.spk_embed_dim} (x-vector {i})")
                first[id(x)] = len(host)
                host.append(v)
            rows.append(first[id(x)])
        if not host:
            raise ValueError("no x-vectors")
        s = torch.from_numpy(np.stack(host)).to(self.dev)
        sn = torch.empty_like(s)
        ops.l2_normalize(s, sn)
        table = torch.empty(len(host), c.adim, dtype=torch.float32, device=self.dev)
        ops.linear_fwd(sn, self.store.p["spk.ws"], table, bias=self.store.p["spk.b"], compute=F32)
        return table, rows

    # ---- the style encoder -----------------------------------------------------------------------------------------------
    def _gst_derived(self):
        """What depends on the weights only, once per load: BatchNorm2d's running statistics folded into (scale, shift) per
        conv layer, and the keys and values of the style tokens, linear_{k,v}(tanh(gst_embs)) [tokens][d] (fp64, then fp32)."""
        if self._gst is None:
            p, buf, out = self.store.p, self.store.buf, {}
            for i in range(len(self.c.gst_conv_chans)):
                n = f"gst.conv.{i}.bn."
                sc = p[n + "g"].double() / torch.sqrt(buf[n + "rv"].double() + 1e-5)
                out[f"scale.{i}"] = sc.float().contiguous()
                out[f"shift.{i}"] = (p[n + "b"].double() - buf[n + "rm"].double() * sc).float().contiguous()
            e = torch.tanh(p["gst.stl.embs"].double())
            for n in ("k", "v"):
                out[n] = (e @ p[f"gst.stl.{n}.w"].double().t() + p[f"gst.stl.{n}.b"].double()).float().contiguous()
            self._gst = out
        return self._gst

    def style_from_mel(self, mel, lens=None, host_lens=None, keep=None):
        """The StyleEncoder over log-mel frames: mel device fp32 [B][T][n_mels], row b valid for its own length and holding
        anything behind it.  lens: device int32 [L + 1][B], row l the rows' time lengths in front of conv layer l (row L: the
        GRU's steps), None when every row is T long.  Returns style [B][d] (a fresh tensor); keep: a dict that receives the last
        conv output [B][T'][F'][C] and ref_embs [B][H] (views of the workspace, valid until the next call).
        len(gst_conv_chans) + 2 launches whatever B is."""
        c, p, ws = self.c, self.store.p, self.ws
        if not c.use_gst:
            raise ValueError("this checkpoint has no GST style encoder")
        if mel.dim() != 3 or mel.shape[2] != c.n_mels or mel.dtype != torch.float32 or not mel.is_contiguous():
            raise ValueError(f"mel must be a contiguous fp32 [B][T][{c.n_mels}] tensor")
        g, plan = self._gst_derived(), c.gst_plan()
        B, T = int(mel.shape[0]), int(mel.shape[1])
        if T < 1:
            raise ValueError("a prompt of no frames")
        k, s, H, d = c.gst_conv_kernel, c.gst_conv_stride, c.gst_gru_units, c.adim
        x = mel.view(B, T, c.n_mels, 1)
        for i, (cin, cout, Fi, Fo) in enumerate(plan):
            To = gst_out_len(T, k, s)
            y = ws.get(f"gst.y{i}", (B, To, Fo, cout))
            ops.gst_conv_bn_relu(x, p[f"gst.conv.{i}.w"], g[f"scale.{i}"], g[f"shift.{i}"], y,
                                 None if lens is None else lens[i], k, s)
            x, T = y, To
        gi = ws.get("gst.gi", (B * T, 3 * H))
        ops.linear_fwd(x.view(B * T, -1), p["gst.gru.wih"], gi, bias=p["gst.gru.bih"], compute=F32)
        ref = ws.get("gst.ref", (B, H))
        style = torch.empty(B, d, dtype=torch.float32, device=self.dev)
        ops.gst_gru_stl(gi.view(B, T, 3 * H), p["gst.gru.whh"], p["gst.gru.bhh"], None if lens is None else lens[len(plan)],
                        p["gst.stl.q.w"], p["gst.stl.q.b"], g["k"], g["v"], p["gst.stl.out.w"], p["gst.stl.out.b"], ref, style,
                        c.gst_heads)
        if keep is not None:
            keep["conv"], keep["ref_embs"] = x, ref
        return style

    def _gst_len_table(self, frames):
        """Device int32 [L + 1][B]: the time lengths of the rows in front of every conv layer and of the GRU, through one
        pinned buffer in one copy that the host does not wait for."""
        c, B = self.c, len(frames)
        L1 = len(c.gst_conv_chans) + 1
        tab = np.zeros((L1, B), np.int32)
        tab[0] = frames
        for l in range(1, L1):
            tab[l] = [gst_out_len(int(n), c.gst_conv_kernel, c.gst_conv_stride) for n in tab[l - 1]]
        if self._gst_lens is None or self._gst_lens[0].numel() < tab.size:
            self._gst_lens = (torch.zeros(2 * tab.size, dtype=torch.int32, pin_memory=True),
                              torch.zeros(2 * tab.size, dtype=torch.int32, device=self.dev), torch.cuda.Event())
        else:       # the previous table must have left the pinned buffer (usually long ago: its style has been used since)
            self._gst_lens[2].synchronize()
        host, dev, copied = self._gst_lens
        host[:tab.size].copy_(torch.from_numpy(tab.reshape(-1)))
        dev[:tab.size].copy_(host[:tab.size], non_blocking=True)
        copied.record()
        return dev[:tab.size].view(L1, B)

    def _prompt_mel(self, wav):
        """(log-mel [1][F][n_mels] on the device, F) of one prompt at its exact length, by the TTS model's own extractor,
        unnormalised, as duration_predict feeds it to the style encoder."""
        w = torch.as_tensor(np.asarray(wav, dtype=np.float32)).reshape(1, -1)
        if w.shape[1] <= self.feats.n_fft // 2:
            raise ValueError(f"a prompt of {w.shape[1]} samples is too short for the extractor's reflect padding")
        mel, _ = self.feats(w)
        return mel, int(mel.shape[1])

    def style_embedding(self, wav):
        """Style embedding of one prompt waveform (1-D, at the extractor's sampling rate): device [1][d]."""
        if not self.c.use_gst:
            raise ValueError("this checkpoint has no GST style encoder")
        mel, _ = self._prompt_mel(wav)
        return self.style_from_mel(mel.contiguous())

    def style_embedding_batch(self, wavs):
        """Style embeddings of several prompts: device [B][d].  Every prompt's log-mel is taken at its exact length (a padded
        batch would reflect at the padded end); the conv layers, the GRU and the token attention then run as ONE ragged pass
        over the mels padded to the longest, row b computed as style_embedding computes it alone."""
        if not self.c.use_gst:
            raise ValueError("this checkpoint has no GST style encoder")
        wavs = list(wavs)
        if not wavs:
            raise ValueError("no prompts")
        if len(wavs) == 1:
            return self.style_embedding(wavs[0])
        mels = [self._prompt_mel(w) for w in wavs]
        frames = [F for _, F in mels]
        x = self.ws.get("gst.mel", (len(wavs), max(frames), self.c.n_mels))
        for b, (m, F) in enumerate(mels):
            x[b, :F].copy_(m[0])
        return self.style_from_mel(x, self._gst_len_table(frames))

    def forward_ids(self, ids, spk_bias=None, style=None):
        """ids: device int64 [T] (eos included); style: device [1][d] from style_embedding (a GST model needs it, another
        model refuses it), added to every encoder output row in front of the x-vector integration.  Returns device tensors
        (hs [T][d], logd [T], frames [T] int64) valid until the next call."""
        c, T = self.c, int(ids.shape[0])
        if not 1 <= T <= c.max_len:
            raise ValueError(f"sequence length {T} outside 1..{c.max_len}")
        if spk_bias is not None and c.spk_embed_dim <= 0:
            raise ValueError("spk_bias given but the checkpoint has no x-vector projection")
        self._check_style(style, 1, None)
        return self._forward(ids, 1, T, None, spk_bias, style, None)

    def _check_style(self, style, B, rows):
        if not self.c.use_gst:
            if style is not None:
                raise ValueError("style given but the checkpoint has no GST style encoder")
            return
        if style is None:
            raise ValueError("a GST model needs style= (style_embedding of the prompt) with every forward")
        if style.dim() != 2 or style.shape[1] != self.c.adim or style.dtype != torch.float32 or not style.is_contiguous():
            raise ValueError(f"style must be a contiguous fp32 [rows][{self.c.adim}] tensor")
        if rows is None and style.shape[0] not in (1, B):
            raise ValueError(f"style has {style.shape[0]} rows for {B} sequences")

    def forward_ids_batch(self, ids, lens, spk_bias=None, style=None, style_rows=None, spk_rows=None):
        """ids: device int64 [B][Tmax] (eos included; entries behind a row's length: any valid id), lens: device int32 [B],
        1 <= lens[b] <= Tmax.  One padded forward whose row b is computed as forward_ids computes it alone at lens[b]
        (ConformerStack.block_fwd with lens); one speaker bias [1][d] for the whole call, or with spk_rows (device int32 [B]) a table
        [S][d] of which sequence b takes row spk_rows[b] (speaker_bias_table).  Returns device tensors (hs [B][Tmax][d],
        logd [B][Tmax], frames [B][Tmax] int64) valid until the next call; entries behind lens[b] are finite and mean nothing
        (hs is 0 there when the predictor's convs have more than one tap).
        style: device [B][d] (row b for sequence b), [1][d] (one prompt for all), or any [S][d] with style_rows, device int32 [B]:
        sequence b takes style row style_rows[b].
        The number of launches does not depend on B."""
        c = self.c
        if ids.dim() != 2 or ids.dtype != torch.int64 or not ids.is_contiguous():
            raise ValueError("ids must be a contiguous int64 [B][Tmax] tensor")
        B, T, d = int(ids.shape[0]), int(ids.shape[1]), c.adim
        if not 1 <= T <= c.max_len:
            raise ValueError(f"sequence length {T} outside 1..{c.max_len}")
        if spk_bias is not None and c.spk_embed_dim <= 0:
            raise ValueError("spk_bias given but the checkpoint has no x-vector projection")
        if spk_rows is not None:
            if spk_bias is None or spk_bias.dim() != 2 or spk_bias.shape[1] != d or spk_bias.dtype != torch.float32 \
                    or not spk_bias.is_contiguous():
                raise ValueError(f"spk_rows needs spk_bias as a contiguous fp32 [speakers][{d}] table")
            if spk_rows.numel() != B:
                raise ValueError(f"spk_rows has {spk_rows.numel()} entries for {B} sequences")
        self._check_style(style, B, style_rows)
        hs, logd, frames = self._forward(ids, B, T, lens, spk_bias, style, style_rows, spk_rows)
        return hs.view(B, T, d), logd.view(B, T), frames.view(B, T)

    def _forward(self, ids, B, T, lens, spk_bias, style, style_rows, spk_rows=None):
        """The body of forward_ids (lens None, B = 1: no padded keys, the plain kernels) and of forward_ids_batch (lens: row b
        as if alone at lens[b]).  spk_rows (device int32 [B]): spk_bias is a table [S][d] and sequence b takes row spk_rows[b];
        that add, like the style's, also lands behind a row's length, so zero_tail stays behind both.
        Returns (hs [B*T][d], logd [B*T], frames [B*T])."""
        c, p, ws = self.c, self.store.p, self.ws
        eng, M, d = self.eng, B * T, c.adim
        if self._tpos0.numel() < M:
            self._tpos0 = torch.zeros(M, dtype=torch.int64, device=self.dev)
        # Embedding * sqrt(d) (+ pe: legacy rel-pos only scales) -- the MLM prologue kernel with no speech frames
        xs = ws.get("emb.xs", (M, d))
        ops.embed_finish_fwd(None, p["temb"], self._seg0, ids, None, self._tpos0[:M], xs, B, 0, T, d, math.sqrt(d))
        keymask = self._keys1[:T].view(1, T) if lens is None else None
        pos = eng.pe[:T]
        x = xs
        for i in range(c.enc_blocks):
            x = eng.block_fwd(f"enc.{i}", x, pos, keymask, B, T, lens=lens)
        hs = eng._ln_fwd("enc.after", x, "enc.after", out_dtype=torch.float32)
        if style is not None:
            ops.gst_add_style(hs, style, B, T, rows=style_rows)
        if spk_bias is not None and spk_rows is not None:
            if c.spk_integration == "add":
                ops.gst_add_style(hs, spk_bias, B, T, rows=spk_rows)
            else:       # projection(cat[hs, s_b]) = hs W_h^T + (W_s s_b + b): the GEMM without bias, then row b's own
                hc = ws.get("spk.hs", (M, d))
                ops.linear_fwd(hs, p["spk.wh"], hc, compute=F32)
                ops.gst_add_style(hc, spk_bias, B, T, rows=spk_rows)
                hs = hc
        elif spk_bias is not None:
            if c.spk_integration == "add":
                ops.bias_act(hs, spk_bias, ACT_NONE)
            else:
                hc = ws.get("spk.hs", (M, d))
                ops.linear_fwd(hs, p["spk.wh"], hc, bias=spk_bias.view(-1), compute=F32)
                hs = hc
        y, pad = hs, (c.dp_kernel - 1) // 2
        tail = lens if pad > 0 else None      # the predictor's convs read zeros behind every row's length
        if tail is not None:
            ops.zero_tail(hs, lens, 1, B, T)
        for l in range(c.dp_layers):
            z = ws.get(f"dp.{l}.z", (M, c.dp_chans))
            ops.conv_fwd(y, p[f"dp.{l}.w"], z, T, pad, bias=p[f"dp.{l}.b"], act=ACT_RELU, compute=F32)
            if l < c.dp_layers - 1:
                y = eng._ln_fwd(f"dp.{l}.ln", z, f"dp.{l}.ln", out_dtype=torch.float32, lens=tail, T=T)
        logd = ws.get("dp.logd", (M,))
        frames = ws.get("dp.frames", (M,), torch.int64)
        l = c.dp_layers - 1
        ops.duration_head(z, p[f"dp.{l}.ln.g"], p[f"dp.{l}.ln.b"], p["dp.lin.w"], p["dp.lin.b"], logd, frames,
                          eps=1e-12, offset=c.dp_offset)
        return hs, logd, frames

    def _chunks(self, lengths, max_score_elems):
        """Indices of `lengths` sorted by length and cut into consecutive chunks with B * H * Tmax^2 <= max_score_elems
        (Tmax = the chunk's longest = last row); a row too long for the cap runs alone."""
        return score_chunks(lengths, self.c.heads, max_score_elems)

    def predict_frames_batch(self, phn_lists, spk_bias=None, max_score_elems: int = 1 << 24, style=None,
                             style_rows=None, spk_rows=None) -> List[np.ndarray]:
        """predict_frames for several phone lists: one int64 array per list (eos entry included), in the order given.
        The ids of all lists go up through one pinned buffer in one copy and all frames come down in one: one host
        synchronisation per call.  The lists are sorted by length and cut into chunks of B rows padded to the chunk's longest,
        each chunk one forward_ids_batch.  max_score_elems caps B * H * Tmax^2 of a chunk, the size of each of the three
        score-sized fp32 tensors of the materialised attention (content scores, position scores, probabilities): the default
        2^24 holds them to 192 MiB together, and e.g. 90 lists of 300 phones at H = 2 still make one chunk.  A list longer
        than the cap allows runs alone.  A chunk of one list, and so a call with one list, takes the B = 1 path of
        predict_frames; every row of a larger chunk is computed as if alone, so the frames do not depend on the chunking.
        style (a GST model): device [len(phn_lists)][d], or [1][d] for one prompt behind all lists, or [S][d] with style_rows, a
        host list naming the style row of every list; the row indices travel with the ids, so a list keeps its style wherever
        the sorting and chunking put it.
        spk_rows (a host list, one entry per list): spk_bias is a table [S][d] (speaker_bias_table) and list i takes its row
        spk_rows[i]; these indices travel the same way, and a chunk of one list runs with that list's row as its one bias."""
        lists = [self.tokens_to_ids(list(ph)) for ph in phn_lists]
        if not lists:
            return []
        krow = None
        if spk_rows is not None:
            krow = [int(r) for r in spk_rows]
            if spk_bias is None or spk_bias.dim() != 2:
                raise ValueError("spk_rows needs spk_bias as a [speakers][d] table")
            if len(krow) != len(lists) or min(krow) < 0 or max(krow) >= spk_bias.shape[0]:
                raise ValueError("spk_rows does not fit the phone lists and the rows of the speaker table")
        bias_of = lambda i: spk_bias if krow is None else spk_bias[krow[i]:krow[i] + 1]
        srow = None
        if style is not None:
            self._check_style(style, len(lists), style_rows)
            srow = [0] * len(lists) if style_rows is None and style.shape[0] == 1 else \
                list(range(len(lists))) if style_rows is None else [int(r) for r in style_rows]
            if len(srow) != len(lists) or min(srow) < 0 or max(srow) >= style.shape[0]:
                raise ValueError("style_rows does not fit the phone lists and the style rows")
        one = lambda i: None if style is None else style[srow[i]:srow[i] + 1]
        if len(lists) == 1:
            return [self.predict_frames(list(phn_lists[0]), bias_of(0), one(0))]
        lengths = [len(x) for x in lists]
        if max(lengths) > self.c.max_len:
            raise ValueError(f"{max(lengths)} tokens: more than max_len {self.c.max_len}")
        chunks = self._chunks(lengths, int(max_score_elems))
        # staging layout (int64 words): per chunk its padded ids [B][Tmax], then all lengths as int32 pairs (with a style:
        # the style rows as int32 behind the lengths, in the same order; with spk_rows: those behind them again)
        offs, n_ids = [], 0
        for ch in chunks:
            offs.append(n_ids)
            n_ids += len(ch) * lengths[ch[-1]]
        o_spk = len(lists) * (1 if style is None else 2)        # (int32 index of the first speaker row)
        n_len = (o_spk + (0 if krow is None else len(lists)) + 1) // 2
        total = n_ids + n_len
        if self._stage_host is None or self._stage_host.numel() < total:
            cap = max(total, 2 * (self._stage_host.numel() if self._stage_host is not None else 0))
            self._stage_host = torch.zeros(cap, dtype=torch.int64, pin_memory=self.dev.type == "cuda")
            self._stage_dev = torch.zeros(cap, dtype=torch.int64, device=self.dev)
        # the pinned staging buffer is free again: the previous call's copy finished before its result reached the host
        host = np.zeros(total, np.int64)
        hl = host[n_ids:].view(np.int32)
        r = 0
        for ch, o in zip(chunks, offs):
            T = lengths[ch[-1]]
            blk = host[o:o + len(ch) * T].reshape(len(ch), T)
            for k, i in enumerate(ch):
                blk[k, :lengths[i]] = lists[i]
                hl[r + k] = lengths[i]
                if style is not None:
                    hl[len(lists) + r + k] = srow[i]
                if krow is not None:
                    hl[o_spk + r + k] = krow[i]
            r += len(ch)
        self._stage_host[:total].copy_(torch.from_numpy(host))
        dev = self._stage_dev[:total]
        dev.copy_(self._stage_host[:total], non_blocking=True)
        dev_lens = dev[n_ids:].view(torch.int32)
        out = self.ws.get("dp.frames.all", (n_ids,), torch.int64)
        r = 0
        for ch, o in zip(chunks, offs):
            B, T = len(ch), lengths[ch[-1]]
            if B == 1:
                _, _, frames = self.forward_ids(dev[o:o + T], bias_of(ch[0]), one(ch[0]))
            else:
                rows = None if style is None else dev_lens[len(lists) + r:len(lists) + r + B]
                krows = None if krow is None else dev_lens[o_spk + r:o_spk + r + B]
                _, _, frames = self.forward_ids_batch(dev[o:o + B * T].view(B, T), dev_lens[r:r + B], spk_bias, style, rows,
                                                      krows)
            out[o:o + B * T].copy_(frames.reshape(-1))
            r += B
        got = out.cpu().numpy()
        res = [None] * len(lists)
        for ch, o in zip(chunks, offs):
            T = lengths[ch[-1]]
            for k, i in enumerate(ch):
                res[i] = got[o + k * T:o + k * T + lengths[i]].copy()
        return res

    def predict_frames(self, phns, spk_bias=None, style=None) -> np.ndarray:
        """Frames per phone of `phns` plus the eos entry (int64, host).  One host synchronisation."""
        ids = self.tokens_to_ids(phns)
        T = len(ids)
        if T > self.c.max_len:
            raise ValueError(f"{T} tokens: more than max_len {self.c.max_len}")
        # the pinned staging buffer is free again: the previous call's copy finished before its result reached the host
        self._ids_host[:T].copy_(torch.as_tensor(ids, dtype=torch.int64))
        dev_ids = self._ids_dev[:T]
        dev_ids.copy_(self._ids_host[:T], non_blocking=True)
        _, _, frames = self.forward_ids(dev_ids, spk_bias, style)
        return frames.cpu().numpy()

    def duration_fn(self, fs: int, hop_length: int, spembs=None):
        """duration_predict(phns, fs, hop_length, ...) of sedit_inference.py:398-425 as a callable for
        SpeechEditor(duration_fn=...): seconds per phone, frames * hop_length / fs in float32 as the reference computes it,
        eos dropped.  spembs=None runs without the x-vector integration, as duration_predict does with sid=None.
        The callable's .batch(list of phone lists) answers several lists from one batched forward (SpeechEditor.plan_batch
        uses it when it is there).

        A GST model's durations depend on the prompt (duration_predict's wav_org), so its callable has needs_prompt = True and
        refuses a bare fn(phns): fn.with_prompt(wav) computes the prompt's style embedding once and returns a plain
        phns -> seconds callable (with .batch) bound to it; fn.batch(phn_lists, prompts=[...]) takes one prompt per list and
        computes one style embedding per distinct prompt OBJECT, all of them in one ragged pass.  fs must be the sampling rate
        of the model's own log-mel extractor.

        A checkpoint with an x-vector projection gives callables (this one, and a GST model's with_prompt one) with
        takes_speaker = True: fn.with_speaker(spembs) is the same callable bound to that x-vector (a GST model's keeps
        needs_prompt / with_prompt), and fn.batch(phn_lists, speakers=[...]) takes one x-vector per list -- one speaker bias per
        distinct OBJECT (speaker_bias_table), all lists still in one ragged forward; an entry of None stands for the callable's
        own spembs.  prompts= and speakers= of a GST model are independent lists of the same length.  speakers=None is the
        one-bias call."""
        bias = self.speaker_bias(spembs) if spembs is not None else None
        hop, fs32 = int(hop_length), np.float32(fs)
        takes = self.c.spk_embed_dim > 0

        def seconds(frames):
            return ((frames * hop).astype(np.float32) / fs32)[:-1].tolist()

        def speaker_args(speakers, n):
            """(spk_bias, spk_rows) of a batch call over n lists."""
            if speakers is None:
                return bias, None
            if not takes:
                raise ValueError("speakers= given, but this checkpoint has no x-vector projection (spk_embed_dim is 0)")
            speakers = list(speakers)
            if len(speakers) != n:
                raise ValueError(f"speakers: {len(speakers)} x-vectors for {n} phone lists")
            for i, x in enumerate(speakers):
                if x is None and spembs is None:
                    raise ValueError(f"speakers[{i}] is None, which stands for the callable's own spembs: it was built without one")
            if not speakers:
                return bias, None
            return self.speaker_bias_table([spembs if x is None else x for x in speakers])

        def speaker_attrs(f, rebind):
            if takes:
                f.takes_speaker = True
                f.with_speaker = rebind
            return f

        if self.c.use_gst:
            if int(fs) != self.feats.fs:
                raise ValueError(f"fs {fs} is not the sampling rate of the checkpoint's log-mel extractor ({self.feats.fs})")

            def with_prompt(wav, _style=None):
                cache = [] if _style is None else _style        # (_style: with_speaker hands the prompt's cache on)

                def style():        # on the first query: a plan that asks for no durations costs no style embedding
                    if not cache:
                        cache.append(self.style_embedding(wav))
                    return cache[0]

                def fn(phns):
                    return seconds(self.predict_frames(list(phns), bias, style()))

                def batch(phn_lists, max_score_elems: int = 1 << 24, speakers=None):
                    phn_lists = list(phn_lists)
                    tab, rows = speaker_args(speakers, len(phn_lists))
                    if rows is None:
                        return [seconds(f) for f in self.predict_frames_batch(phn_lists, bias, max_score_elems, style())]
                    return [seconds(f) for f in self.predict_frames_batch(phn_lists, tab, max_score_elems, style(), None, rows)]
                fn.batch = batch
                return speaker_attrs(fn, lambda x: self.duration_fn(fs, hop_length, x).with_prompt(wav, cache))

            def fn(phns):
                raise ValueError("the durations of a GST model depend on the prompt: use with_prompt(wav)(phns) or "
                                 "batch(phn_lists, prompts=[...])")

            def batch(phn_lists, prompts=None, max_score_elems: int = 1 << 24, speakers=None):
                """One list of seconds per phone list; prompts: one waveform per list (the same object may repeat); speakers:
                one x-vector per list, likewise."""
                phn_lists = list(phn_lists)
                if prompts is None or len(prompts) != len(phn_lists):
                    raise ValueError("a GST model needs prompts=[...], one prompt waveform per phone list")
                tab, srows = speaker_args(speakers, len(phn_lists))
                if not phn_lists:
                    return []
                first = {}
                rows = [first.setdefault(id(w), len(first)) for w in prompts]
                distinct = [None] * len(first)
                for w, r in zip(prompts, rows):
                    distinct[r] = w
                style = self.style_embedding_batch(distinct)
                if srows is None:
                    return [seconds(f) for f in self.predict_frames_batch(phn_lists, bias, max_score_elems, style, rows)]
                return [seconds(f) for f in self.predict_frames_batch(phn_lists, tab, max_score_elems, style, rows, srows)]
            fn.needs_prompt = True
            fn.with_prompt = with_prompt
            fn.batch = batch
            return speaker_attrs(fn, lambda x: self.duration_fn(fs, hop_length, x))

        def fn(phns):
            return seconds(self.predict_frames(list(phns), bias))

        def batch(phn_lists, max_score_elems: int = 1 << 24, speakers=None):
            """One list of seconds per phone list, from one predict_frames_batch call (one host synchronisation); speakers:
            one x-vector per list (the same object may repeat)."""
            phn_lists = list(phn_lists)
            tab, rows = speaker_args(speakers, len(phn_lists))
            if rows is None:
                return [seconds(f) for f in self.predict_frames_batch(phn_lists, bias, max_score_elems)]
            return [seconds(f) for f in self.predict_frames_batch(phn_lists, tab, max_score_elems, None, None, rows)]
        fn.batch = batch
        return speaker_attrs(fn, lambda x: self.duration_fn(fs, hop_length, x))

