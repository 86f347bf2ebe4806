"""Conformer FastSpeech2 duration model on the device: the phone durations of the speech-editing driver.

The reference asks the user's own torch FastSpeech2 for them (espnet2/bin/sedit_inference.py:398-425 duration_predict,
twice per edit with duration_adjust).  Only the part of FastSpeech2 that duration_predict runs is built here:
  - the text encoder (espnet/nets/pytorch_backend/conformer/encoder.py with an Embedding input layer): Embedding * sqrt(d)
    (LegacyRelPositionalEncoding), the Conformer blocks of MLMEngine.block_fwd, after_norm;
  - the x-vector integration (espnet2/tts/fastspeech2/fastspeech2.py:784-808, "add" or "concat");
  - the DurationPredictor (espnet/nets/pytorch_backend/fastspeech/duration_predictor.py) in inference mode: k-tap convs
    with ReLU and LayerNorm, then a3t_duration_head (last LayerNorm, Linear(C -> 1), clamp(round(exp(x) - offset), 0)).
fp32 compute, eval mode.  A single phone sequence runs as its own B = 1 forward at its exact length n + 1 (the appended eos):
legacy rel-pos attention reads pe[:T] and the conv module does not mask padded frames, so plain padding would change the
result.  Several sequences run as ONE padded forward with per-row lengths (forward_ids_batch): the engine's ragged block
forward gives every row what it would get alone -- rel_shift at the row's own length, zeros behind it for every k-tap conv.
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
from .engine import MLMEngine, Workspace
from .params import ParamStore, _block_layout, _ref_block_map

# FastSpeech2.__init__ defaults (espnet2/tts/fastspeech2/fastspeech2.py) of the keys the duration path reads
_FS2_DEFAULTS = dict(adim=384, aheads=4, elayers=6, eunits=1536, positionwise_layer_type="conv1d",
                     positionwise_conv_kernel_size=1, encoder_normalize_before=True, encoder_concat_after=False,
                     encoder_type="transformer", conformer_rel_pos_type="legacy", conformer_pos_enc_layer_type="rel_pos",
                     conformer_self_attn_layer_type="rel_selfattn", conformer_activation_type="swish",
                     use_macaron_style_in_conformer=True, use_cnn_in_conformer=True, zero_triu=False,
                     conformer_enc_kernel_size=7, duration_predictor_layers=2, duration_predictor_chans=384,
                     duration_predictor_kernel_size=3, spk_embed_dim=None, spk_embed_integration_type="add",
                     use_gst=False)

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

    @staticmethod
    def from_espnet(conf: Dict[str, Any]) -> "FS2DurationConfig":
        """Translate an ESPnet TTS config.yaml (tts: fastspeech2, tts_conf, token_list)."""
        if conf.get("tts", "fastspeech2") != "fastspeech2":
            raise NotImplementedError(f"tts: {conf.get('tts')!r}: only fastspeech2 is implemented")
        tl = list(conf.get("token_list") or [])
        if not tl:
            raise ValueError("config has no token_list")
        t = dict(_FS2_DEFAULTS)
        t.update(conf.get("tts_conf") or {})
        if t["use_gst"]:
            raise NotImplementedError("use_gst: true (the GST style encoder) is not implemented")
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
        return FS2DurationConfig(vocab=len(tl), adim=t["adim"], heads=t["aheads"], ff=t["eunits"],
                                 ff_kernel=t["positionwise_conv_kernel_size"], enc_blocks=t["elayers"],
                                 enc_kernel=t["conformer_enc_kernel_size"], dp_layers=t["duration_predictor_layers"],
                                 dp_chans=t["duration_predictor_chans"], dp_kernel=t["duration_predictor_kernel_size"],
                                 spk_embed_dim=spk, spk_integration=t["spk_embed_integration_type"], token_list=tl,
                                 dropout_rate=0.0, positional_dropout_rate=0.0, attention_dropout_rate=0.0)


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
    return lay


def buffer_layout(c: FS2DurationConfig):
    lay = {}
    for i in range(c.enc_blocks):
        lay[f"enc.{i}.cnv.bn.rm"] = (c.adim,)
        lay[f"enc.{i}.cnv.bn.rv"] = (c.adim,)
    return lay


def key_map(c: FS2DurationConfig):
    """(ESPnet TTS checkpoint key, store name, (column slice) | None, kind): ParamStore's kinds, plus "cols"."""
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
                        if k.startswith(("tts.encoder.", "tts.duration_predictor.", "tts.projection.", "tts.gst.")))
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
        dst.copy_(src.reshape(dst.shape).to(device=store.device, dtype=torch.float32))


class _RowWorkspace(Workspace):
    """Workspace whose buffers keep their storage across sequence lengths: one grow-only allocation per (name, dtype),
    viewed at the requested shape (the engine's Workspace would keep one buffer set per distinct length)."""

    def __init__(self, device):
        super().__init__(device)
        self.shapes = {}

    def get(self, name, shape, dtype=torch.float32, zero=False, zero_once=False):
        shape = tuple(shape)
        n, key = math.prod(shape), (name, dtype)
        t = self.bufs.get(key)
        if t is None or t.numel() < n:
            t = torch.zeros(max(n, 1), dtype=dtype, device=self.device)
            self.bufs[key] = t
            self.shapes.pop(key, None)
        v = t[:n].view(shape)
        if zero or (zero_once and self.shapes.get(key) != shape):
            v.zero_()
        self.shapes[key] = shape
        return v


class FS2DurationModel:
    """The duration path of a conformer FastSpeech2 checkpoint on one device (fp32, eval mode)."""

    def __init__(self, cfg: FS2DurationConfig, device="cuda"):
        self.c = cfg
        self.store = ParamStore(cfg, device, layout=param_layout(cfg), buffers=buffer_layout(cfg), keymap=key_map(cfg))
        self.dev = self.store.device
        self.eng = MLMEngine(cfg, self.store, compute="f32", training=False)
        self.eng.ws = _RowWorkspace(self.dev)
        self.ws = self.eng.ws
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

    # ---- loading ---------------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd):
        load_into(self.store, self.c, sd)
        return self

    @staticmethod
    def from_file(config_file: Optional[str], model_file: str, device="cuda") -> "FS2DurationModel":
        """As espnet2's Text2Speech(train_config, model_file): config_file=None reads config.yaml next to model_file."""
        import yaml
        if config_file is None:
            config_file = os.path.join(os.path.dirname(os.path.abspath(model_file)), "config.yaml")
        with open(config_file) as f:
            conf = yaml.safe_load(f)
        model = FS2DurationModel(FS2DurationConfig.from_espnet(conf), device)
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

    def forward_ids(self, ids, spk_bias=None):
        """ids: device int64 [T] (eos included).  Returns device tensors (hs [T][d], logd [T], frames [T] int64) valid
        until the next call."""
        c, p, ws = self.c, self.store.p, self.ws
        T, d = int(ids.shape[0]), c.adim
        if not 1 <= T <= c.max_len:
            raise ValueError(f"sequence length {T} outside 1..{c.max_len}")
        if spk_bias is not None and c.spk_embed_dim <= 0:
            raise ValueError("spk_bias given but the checkpoint has no x-vector projection")
        eng = self.eng
        # Embedding * sqrt(d) (+ pe: legacy rel-pos only scales) -- the MLM prologue kernel with no speech frames
        xs = ws.get("emb.xs", (T, d))
        ops.embed_finish_fwd(None, p["temb"], self._seg0, ids, None, self._tpos0, xs, 1, 0, T, d, math.sqrt(d))
        keymask = self._keys1[:T].view(1, T)
        pos = eng.pe[:T]
        x = xs
        for i in range(c.enc_blocks):
            x = eng.block_fwd(f"enc.{i}", x, pos, keymask, 1, T)
        hs = eng._ln_fwd("enc.after", x, "enc.after", out_dtype=torch.float32)
        if spk_bias is not None:
            if c.spk_integration == "add":
                ops.bias_act(hs, spk_bias, ACT_NONE)
            else:
                hc = ws.get("spk.hs", (T, d))
                ops.linear_fwd(hs, p["spk.wh"], hc, bias=spk_bias.view(-1), compute=F32)
                hs = hc
        y, pad = hs, (c.dp_kernel - 1) // 2
        for l in range(c.dp_layers):
            z = ws.get(f"dp.{l}.z", (T, c.dp_chans))
            ops.conv_fwd(y, p[f"dp.{l}.w"], z, T, pad, bias=p[f"dp.{l}.b"], act=ACT_RELU, compute=F32)
            if l < c.dp_layers - 1:
                y = eng._ln_fwd(f"dp.{l}.ln", z, f"dp.{l}.ln", out_dtype=torch.float32)
        logd = ws.get("dp.logd", (T,))
        frames = ws.get("dp.frames", (T,), torch.int64)
        l = c.dp_layers - 1
        ops.duration_head(z, p[f"dp.{l}.ln.g"], p[f"dp.{l}.ln.b"], p["dp.lin.w"], p["dp.lin.b"], logd, frames,
                          eps=1e-12, offset=c.dp_offset)
        return hs, logd, frames

    def forward_ids_batch(self, ids, lens, spk_bias=None):
        """ids: device int64 [B][Tmax] (eos included; entries behind a row's length: any valid id), lens: device int32 [B],
        1 <= lens[b] <= Tmax.  One padded forward whose row b is computed as forward_ids computes it alone at lens[b]
        (MLMEngine.block_fwd with lens); one speaker bias for the whole call.  Returns device tensors (hs [B][Tmax][d],
        logd [B][Tmax], frames [B][Tmax] int64) valid until the next call; entries behind lens[b] are finite and mean nothing
        (hs is 0 there when the predictor's convs have more than one tap).
        The number of launches does not depend on B."""
        c, p, ws = self.c, self.store.p, self.ws
        if ids.dim() != 2 or ids.dtype != torch.int64 or not ids.is_contiguous():
            raise ValueError("ids must be a contiguous int64 [B][Tmax] tensor")
        B, T, d = int(ids.shape[0]), int(ids.shape[1]), c.adim
        if not 1 <= T <= c.max_len:
            raise ValueError(f"sequence length {T} outside 1..{c.max_len}")
        if spk_bias is not None and c.spk_embed_dim <= 0:
            raise ValueError("spk_bias given but the checkpoint has no x-vector projection")
        eng, M = self.eng, B * T
        if self._tpos0.numel() < M:
            self._tpos0 = torch.zeros(M, dtype=torch.int64, device=self.dev)
        tpos = self._tpos0[:M]
        xs = ws.get("emb.xs", (M, d))
        ops.embed_finish_fwd(None, p["temb"], self._seg0, ids, None, tpos, xs, B, 0, T, d, math.sqrt(d))
        pos = eng.pe[:T]
        x = xs
        for i in range(c.enc_blocks):
            x = eng.block_fwd(f"enc.{i}", x, pos, None, B, T, lens=lens)
        hs = eng._ln_fwd("enc.after", x, "enc.after", out_dtype=torch.float32)
        if spk_bias is not None:
            if c.spk_integration == "add":
                ops.bias_act(hs, spk_bias, ACT_NONE)
            else:
                hc = ws.get("spk.hs", (M, d))
                ops.linear_fwd(hs, p["spk.wh"], hc, bias=spk_bias.view(-1), compute=F32)
                hs = hc
        y, pad = hs, (c.dp_kernel - 1) // 2
        if pad > 0:      # the predictor's first conv reads zeros behind every row's length
            ops.zero_tail(hs, lens, 1, B, T)
        for l in range(c.dp_layers):
            z = ws.get(f"dp.{l}.z", (M, c.dp_chans))
            ops.conv_fwd(y, p[f"dp.{l}.w"], z, T, pad, bias=p[f"dp.{l}.b"], act=ACT_RELU, compute=F32)
            if l < c.dp_layers - 1:
                y = eng._ln_fwd(f"dp.{l}.ln", z, f"dp.{l}.ln", out_dtype=torch.float32,
                                lens=lens if pad > 0 else None, T=T)
        logd = ws.get("dp.logd", (M,))
        frames = ws.get("dp.frames", (M,), torch.int64)
        l = c.dp_layers - 1
        ops.duration_head(z, p[f"dp.{l}.ln.g"], p[f"dp.{l}.ln.b"], p["dp.lin.w"], p["dp.lin.b"], logd, frames,
                          eps=1e-12, offset=c.dp_offset)
        return hs.view(B, T, d), logd.view(B, T), frames.view(B, T)

    def _chunks(self, lengths, max_score_elems):
        """Indices of `lengths` sorted by length and cut into consecutive chunks with B * H * Tmax^2 <= max_score_elems
        (Tmax = the chunk's longest = last row); a row too long for the cap runs alone."""
        order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
        H, out, cur = self.c.heads, [], []
        for i in order:
            if cur and (len(cur) + 1) * H * lengths[i] ** 2 > max_score_elems:
                out.append(cur)
                cur = []
            cur.append(i)
        if cur:
            out.append(cur)
        return out

    def predict_frames_batch(self, phn_lists, spk_bias=None, max_score_elems: int = 1 << 24) -> List[np.ndarray]:
        """predict_frames for several phone lists: one int64 array per list (eos entry included), in the order given.
        The ids of all lists go up through one pinned buffer in one copy and all frames come down in one: one host
        synchronisation per call.  The lists are sorted by length and cut into chunks of B rows padded to the chunk's longest,
        each chunk one forward_ids_batch.  max_score_elems caps B * H * Tmax^2 of a chunk, the size of each of the three
        score-sized fp32 tensors of the materialised attention (content scores, position scores, probabilities): the default
        2^24 holds them to 192 MiB together, and e.g. 90 lists of 300 phones at H = 2 still make one chunk.  A list longer
        than the cap allows runs alone.  A chunk of one list, and so a call with one list, takes the B = 1 path of
        predict_frames; every row of a larger chunk is computed as if alone, so the frames do not depend on the chunking."""
        lists = [self.tokens_to_ids(list(ph)) for ph in phn_lists]
        if not lists:
            return []
        if len(lists) == 1:
            return [self.predict_frames(list(phn_lists[0]), spk_bias)]
        lengths = [len(x) for x in lists]
        if max(lengths) > self.c.max_len:
            raise ValueError(f"{max(lengths)} tokens: more than max_len {self.c.max_len}")
        chunks = self._chunks(lengths, int(max_score_elems))
        # staging layout (int64 words): per chunk its padded ids [B][Tmax], then all lengths as int32 pairs
        offs, n_ids = [], 0
        for ch in chunks:
            offs.append(n_ids)
            n_ids += len(ch) * lengths[ch[-1]]
        n_len = (len(lists) + 1) // 2
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
                _, _, frames = self.forward_ids(dev[o:o + T], spk_bias)
            else:
                _, _, frames = self.forward_ids_batch(dev[o:o + B * T].view(B, T), dev_lens[r:r + B], spk_bias)
            out[o:o + B * T].copy_(frames.reshape(-1))
            r += B
        got = out.cpu().numpy()
        res = [None] * len(lists)
        for ch, o in zip(chunks, offs):
            T = lengths[ch[-1]]
            for k, i in enumerate(ch):
                res[i] = got[o + k * T:o + k * T + lengths[i]].copy()
        return res

    def predict_frames(self, phns, spk_bias=None) -> np.ndarray:
        """Frames per phone of `phns` plus the eos entry (int64, host).  One host synchronisation."""
        ids = self.tokens_to_ids(phns)
        T = len(ids)
        if T > self.c.max_len:
            raise ValueError(f"{T} tokens: more than max_len {self.c.max_len}")
        # the pinned staging buffer is free again: the previous call's copy finished before its result reached the host
        self._ids_host[:T].copy_(torch.as_tensor(ids, dtype=torch.int64))
        dev_ids = self._ids_dev[:T]
        dev_ids.copy_(self._ids_host[:T], non_blocking=True)
        _, _, frames = self.forward_ids(dev_ids, spk_bias)
        return frames.cpu().numpy()

    def duration_fn(self, fs: int, hop_length: int, spembs=None):
        """duration_predict(phns, fs, hop_length, ...) of sedit_inference.py:398-425 as a callable for
        SpeechEditor(duration_fn=...): seconds per phone, frames * hop_length / fs in float32 as the reference computes it,
        eos dropped.  spembs=None runs without the x-vector integration, as duration_predict does with sid=None.
        The callable's .batch(list of phone lists) answers several lists from one batched forward (SpeechEditor.plan_batch
        uses it when it is there)."""
        bias = self.speaker_bias(spembs) if spembs is not None else None
        hop, fs32 = int(hop_length), np.float32(fs)

        def seconds(frames):
            return ((frames * hop).astype(np.float32) / fs32)[:-1].tolist()

        def fn(phns):
            return seconds(self.predict_frames(list(phns), bias))

        def batch(phn_lists, max_score_elems: int = 1 << 24):
            """One list of seconds per phone list, from one predict_frames_batch call (one host synchronisation)."""
            return [seconds(f) for f in self.predict_frames_batch(list(phn_lists), bias, max_score_elems)]
        fn.batch = batch
        return fn
