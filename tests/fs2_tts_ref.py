"""CPU restatement of FastSpeech2's text-to-mel inference (espnet2/tts/fastspeech2/fastspeech2.py:614-782 behind
espnet2/tts/espnet_model.py:223-308) over a padded batch with per-row lengths ("ragged" semantics): the yardstick of
a3t_amd/fs2_tts.py and a3t_amd/csrc/fs2_tts.hip, held to the reference's own outputs in tests/golden/fs2_tts.{npz,json}.

Row b of a padded batch gets what it would get alone:
  1. the text side (encoder, style, x-vector integration, duration predictor) follows tests/fs2_ragged_ref.py's rule, with its
     attention, FFN and conv module;
  2. the pitch and energy predictors read zeros behind the row's token count n_b, as the duration predictor does, and the
     embedding convolutions read pitch = energy = 0 outside [0, n_b);
  3. the length regulator repeats token t of row b d'[b][t] times (d' = round-half-even(d * alpha) in fp32 when alpha != 1),
     F_b = sum d' frames, zeros behind;
  4. the decoder blocks mask keys >= F_b, take the legacy rel_shift at F_b and feed zeros behind F_b to every k-tap conv;
  5. every postnet convolution reads zeros behind F_b (BatchNorm's shift makes the tail non-zero after each layer);
  6. feat_gen = before + postnet(before), feat_gen_denorm = feat_gen * std + mean, rows behind F_b are 0.
Also here: the fixture's documented weight overrides, its inputs from seeds and its GlobalMVN statistics.  Not a test module:
tests/test_fs2_tts_host.py and tests/test_gpu_fs2_tts.py import it, tests/golden/make_golden_fs2_tts.py takes the inputs and
the overrides from here.  Nothing of the reference is imported."""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import fs2_ragged_ref as RR
import gst_ref as GR
from oracle import a3t_oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- the fixture's inputs and overrides --------------------------------------------------------------------------------
LENGTHS = (2, 7, 33, 130)
ALPHA_CASE, ALPHA = ("plain", 33), 1.3          # the (model, length) that is also run at alpha = 1.3
PROMPT_FRAMES = 131                             # the GST model's prompt: gst_ref.mel_input(PROMPT_FRAMES, seed)
STATS_SEED = 5150
TIE_MARGIN = 0.02
OVERRIDES = {
    "duration_predictor.linear.bias": "a constant per model (JSON: dp_bias): centres the durations so that every case has "
                                      "tokens of 0 frames and of >= 3 frames",
    "duration_predictor.linear.weight": "x dp_scale (JSON): widens the spread of the log-domain durations",
    "duration_predictor.conv.{l}.2.weight": "make_golden_fs2.apply_overrides (LayerNorm gammas)",
    "{pitch,energy}_predictor.linear.weight": "x VAR_SCALE: predictions of order 1, so that the embeddings move hs",
    "postnet.postnet.{l}.0.weight": "x POST_SCALE: keeps the signal through the tanh stack, so that the postnet moves the mel",
}
VAR_SCALE, POST_SCALE = 8.0, 2.0


def apply_tts_overrides(state, conf, dp_bias, dp_scale):
    """The documented overrides on a procedural_state dict keyed by the FastSpeech2 state-dict names (after
    make_golden_fs2.apply_overrides and, for a GST model, gst_ref.apply_gst_overrides)."""
    state["duration_predictor.linear.bias"] = np.full((1,), dp_bias, np.float32)
    k = "duration_predictor.linear.weight"
    state[k] = (state[k] * np.float32(dp_scale)).astype(np.float32)
    for v in ("pitch", "energy"):
        k = f"{v}_predictor.linear.weight"
        state[k] = (state[k] * np.float32(VAR_SCALE)).astype(np.float32)
    for l in range(conf.get("postnet_layers", 5)):
        k = f"postnet.postnet.{l}.0.weight"
        state[k] = (state[k] * np.float32(POST_SCALE)).astype(np.float32)
    return state


def build_state(shapes, conf, seed, dp_bias, dp_scale):
    """The fixture's checkpoint of one model as numpy arrays under the FastSpeech2 names."""
    state = O.procedural_state({k: tuple(v) for k, v in shapes.items()}, seed)
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden_fs2 import apply_overrides      # (imports nothing of the reference)
    apply_overrides(state, conf.get("duration_predictor_layers", 2))
    if conf.get("use_gst"):
        GR.apply_gst_overrides(state, conf.get("gst_conv_layers", 6))
    return apply_tts_overrides(state, conf, dp_bias, dp_scale)


def mvn_stats(n_mels=80, seed=STATS_SEED):
    """A feats_stats.npz as ESPnet's collect_stats writes it (count, sum, sum_square) for log-mels of the kind
    gst_ref.mel_input draws: float64 arrays."""
    rs = np.random.RandomState(seed)
    count = 48211
    mean = -2.0 + np.linspace(0.5, -2.5, n_mels) + rs.uniform(-0.2, 0.2, n_mels)
    std = rs.uniform(0.7, 1.4, n_mels)
    return dict(count=np.array(count, np.int64), sum=mean * count, sum_square=(std * std + mean * mean) * count)


def mvn_mean_std(stats, norm_means=True, norm_vars=True, eps=1e-20):
    """GlobalMVN.__init__ (espnet2/layers/global_mvn.py:41-57): (mean, std) in float64; None where the flag is off."""
    count = stats["count"]
    mean = stats["sum"] / count
    var = stats["sum_square"] / count - mean * mean
    std = np.sqrt(np.maximum(var, eps))
    return (mean if norm_means else None), (std if norm_vars else None)


def meta():
    return json.load(open(os.path.join(G, "fs2_tts.json")))


def arrays():
    return np.load(os.path.join(G, "fs2_tts.npz"))


def stats_file():
    return os.path.join(G, "fs2_tts_stats.npz")


def checkpoint(m, case):
    """(ESPnet config dict, state dict under the FastSpeech2 names without 'tts.') of a fixture model."""
    mc = m["cases"][case]
    state = build_state(mc["shapes"], mc["tts_conf"], mc["seed"], mc["dp_bias"], mc["dp_scale"])
    cfg = {"tts": "fastspeech2", "tts_conf": mc["tts_conf"], "token_list": m["token_list"], "feats_extract": "fbank",
           "feats_extract_conf": m["feats_extract_conf"]}
    if mc.get("normalize"):
        cfg["normalize"] = "global_mvn"
        cfg["normalize_conf"] = {"stats_file": stats_file()}
    return cfg, {k: torch.from_numpy(np.array(v)) for k, v in state.items()}


def token_ids(T, seed, vocab):
    """T - 1 random phone ids (never <blank>, <unk> or eos) + eos."""
    rs = np.random.RandomState(3000 + 17 * T + seed)
    return np.concatenate([rs.randint(2, vocab - 1, size=T - 1), [vocab - 1]]).astype(np.int64)


def scale_of(a):
    return max(1.0, float(np.abs(np.asarray(a)).max()))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def variance_predictor(p, name, hs, mask, conf):
    """VariancePredictor (espnet/nets/pytorch_backend/fastspeech/variance_predictor.py) in eval mode: [B][T]."""
    n_layers = conf.get(f"{name}_predictor_layers", 2)
    pad = (conf.get(f"{name}_predictor_kernel_size", 3) - 1) // 2
    y = (hs * mask).transpose(1, 2)
    for l in range(n_layers):
        pre = f"{name}_predictor.conv.{l}."
        y = torch.relu(F.conv1d(y, p[pre + "0.weight"], p[pre + "0.bias"], padding=pad))
        y = F.layer_norm(y.transpose(1, 2), (y.shape[1],), p[pre + "2.weight"], p[pre + "2.bias"], 1e-12)
        y = (y * mask if l < n_layers - 1 else y).transpose(1, 2)
    return F.linear(y.transpose(1, 2), p[f"{name}_predictor.linear.weight"], p[f"{name}_predictor.linear.bias"]).squeeze(-1)


def variance_embed(hs, pitch, energy, wp, bp, we, be, lens):
    """hs [B][T][d] + energy_embed(energy) + pitch_embed(pitch) for t < lens[b] (the other rows as they are); wp / we are
    Conv1d(1 -> d, k) weights [d][1][k]; pitch / energy [B][T] count as 0 outside [0, lens[b])."""
    B, T, _ = hs.shape
    keep = _mask(lens, T, hs)[:, :, 0] > 0
    zero = torch.zeros((), dtype=hs.dtype, device=hs.device)
    emb = lambda v, w, b: F.conv1d(torch.where(keep, v, zero)[:, None], w, b, padding=(w.shape[2] - 1) // 2).transpose(1, 2)
    out = hs + emb(energy, we, be) + emb(pitch, wp, bp)
    return torch.where(keep[:, :, None], out, hs)


def scale_durations(d, alpha):
    """LengthRegulator's alpha (length_regulator.py:52-54) on an int64 tensor."""
    return d if alpha == 1.0 else torch.round(d.float() * alpha).long()


def kernel_offsets(d, alpha):
    """a3t_length_offsets' arithmetic in numpy on one row of durations: d' = (int) rintf((float) d * (float) alpha) -- ONE
    fp32 product, round half to even -- when alpha != 1, then exclusive int32 prefix sums with the total at the end."""
    d = np.asarray(d, np.int64)
    if np.float32(alpha) != np.float32(1.0):
        d = np.rint(d.astype(np.float32) * np.float32(alpha)).astype(np.int64)
    off = np.zeros(d.shape[0] + 1, np.int32)
    off[1:] = np.cumsum(d).astype(np.int32)
    return d, off


def length_offsets(d, lens, alpha=1.0):
    """d int64 [B][T] -> (scaled durations int64 [B][T] with 0 behind lens[b], exclusive offsets int32 [B][T + 1])."""
    B, T = d.shape
    keep = _mask(lens, T, d)[:, :, 0] > 0
    ds = torch.where(keep, scale_durations(d, alpha), torch.zeros((), dtype=torch.int64, device=d.device))
    off = torch.zeros(B, T + 1, dtype=torch.int32, device=d.device)
    off[:, 1:] = torch.cumsum(ds, 1).to(torch.int32)
    return ds, off


def length_expand(hs, ds, Fp=None, scale=1.0):
    """hs [B][T][d], ds int64 [B][T] (0 behind the row's length) -> ([B][Fp][d], frame counts)."""
    B, _, d = hs.shape
    rows = [torch.repeat_interleave(hs[b], ds[b], dim=0) for b in range(B)]
    lens = [int(r.shape[0]) for r in rows]
    out = torch.zeros(B, max(lens) if Fp is None else Fp, d, dtype=hs.dtype, device=hs.device)
    for b, r in enumerate(rows):
        out[b, :lens[b]] = r * scale
    return out, lens


def _mask(lens, T, like):
    """[B][T][1] of like's dtype and device: 1 for t < lens[b]."""
    return RR._row_mask(lens, T, like.dtype).to(like.device)


def conformer_stack(p, prefix, n_blocks, c, K, x, lens):
    """n_blocks Conformer blocks with the ragged rule of fs2_ragged_ref (its attention, FFN and conv module) and after_norm,
    over x [B][T][d] that LegacyRelPositionalEncoding has already scaled."""
    T = x.shape[1]
    mask = _mask(lens, T, x)
    pos = O.legacy_pe(c, T, x.dtype)[None].to(x.device)
    for i in range(n_blocks):
        pre = f"{prefix}.encoders.{i}."
        x = x + 0.5 * RR._ffn(O._ln(x, p, pre + "norm_ff_macaron", 1e-12), mask, p, pre + "feed_forward_macaron.", c)
        x = x + RR._attention(O._ln(x, p, pre + "norm_mha", 1e-12), pos, lens, p, pre + "self_attn.", c)
        x = x + RR._conv_module(O._ln(x, p, pre + "norm_conv", 1e-12), mask, p, pre + "conv_module.", K)
        x = x + 0.5 * RR._ffn(O._ln(x, p, pre + "norm_ff", 1e-12), mask, p, pre + "feed_forward.", c)
        x = O._ln(x, p, pre + "norm_final", 1e-12)
    return O._ln(x, p, prefix + ".after_norm", 1e-12)


def decoder(p, conf, x, lens):
    """The conformer decoder (input_layer None: LegacyRelPositionalEncoding scales by sqrt(d)) over [B][F][d], rows valid for
    lens[b] frames; after_norm included."""
    d = x.shape[2]
    c = O.A3TConfig(adim=d, heads=conf["aheads"], ff=conf.get("dunits", 1536), ff_kernel=conf["positionwise_conv_kernel_size"])
    return conformer_stack(p, "decoder", conf.get("dlayers", 6), c, conf.get("conformer_dec_kernel_size", 31),
                           x * math.sqrt(d), lens)


def postnet(p, conf, before, lens):
    """Postnet (espnet/nets/pytorch_backend/tacotron2/decoder.py:150-267) in eval mode over [B][F][odim]."""
    n = conf.get("postnet_layers", 5)
    mask = _mask(lens, before.shape[1], before).transpose(1, 2)
    x = before.transpose(1, 2)
    pad = (conf.get("postnet_filts", 5) - 1) // 2
    for l in range(n):
        pre = f"postnet.postnet.{l}."
        x = F.conv1d(x * mask, p[pre + "0.weight"], None, padding=pad)
        x = O._batch_norm(x, p, pre + "1", False)
        if l < n - 1:
            x = torch.tanh(x)
    return x.transpose(1, 2)


def finish(before, post, lens, mean=None, std=None):
    """(feat_gen, feat_gen_denorm or None): before + post, GlobalMVN.inverse, rows behind lens[b] zero."""
    mask = _mask(lens, before.shape[1], before)
    after = (before if post is None else before + post) * mask
    if mean is None and std is None:
        return after, None
    dn = after
    if std is not None:
        dn = dn * torch.as_tensor(std).to(before.device, before.dtype)
    if mean is not None:
        dn = dn + torch.as_tensor(mean).to(before.device, before.dtype)
    return after, dn * mask


def normalize_mel(mel, mean, std):
    """GlobalMVN.forward on [T][n_mels]."""
    x = torch.as_tensor(mel)
    if mean is not None:
        x = x - torch.as_tensor(mean).to(x.device, x.dtype)
    if std is not None:
        x = x / torch.as_tensor(std).to(x.device, x.dtype)
    return x


def synthesize(p, conf, ids, lens, spembs=None, prompt_mel=None, alpha=1.0, mean=None, std=None, dtype=torch.float32,
               durations=None):
    """p: state dict under the FastSpeech2 names; ids [B][Tmax] int64, lens list; prompt_mel (a GST model): the RAW log-mel
    [F][n_mels] of the one prompt behind all rows, normalised here as espnet_model.py:255-262 does.  durations (int64 [B][Tmax]):
    taken instead of the restatement's own (the fp64 run of a test takes the fp32 ones).
    Returns a dict of tensors over the padded batch: duration [B][T] (unscaled, as the reference returns it), pitch, energy [B][T],
    hs_embed [B][T][d], regulated [B][Fmax][d], before / feat_gen / feat_gen_denorm [B][Fmax][odim], and frame_lens (list)."""
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}
    dev = p["feat_out.weight"].device            # (the latency tool puts the weights on the GPU)
    ids = (ids if torch.is_tensor(ids) else torch.as_tensor(np.asarray(ids))).to(dev)
    B, T = ids.shape
    lens = [int(n) for n in lens]
    style = None
    if conf.get("use_gst"):
        mel = prompt_mel if torch.is_tensor(prompt_mel) else torch.as_tensor(np.asarray(prompt_mel))
        mel = normalize_mel(mel.to(dev, dtype), mean, std)
        style = GR.style_encoder(p, conf, mel[None])[2]
    hs, logd = ragged_text(p, conf, ids, lens, spembs, style, dtype)
    mask = _mask(lens, T, hs)
    d = RR.frames_of(logd) if durations is None else torch.as_tensor(durations).to(dev)
    pitch = variance_predictor(p, "pitch", hs, mask, conf)
    energy = variance_predictor(p, "energy", hs, mask, conf)
    hs_e = variance_embed(hs, pitch, energy, p["pitch_embed.0.weight"], p["pitch_embed.0.bias"], p["energy_embed.0.weight"],
                          p["energy_embed.0.bias"], lens)
    ds, _ = length_offsets(d, lens, alpha)
    reg, flens = length_expand(hs_e, ds)
    if min(flens) < 1:
        raise ValueError("a row whose durations sum to 0")
    zs = decoder(p, conf, reg, flens)
    before = F.linear(zs, p["feat_out.weight"], p["feat_out.bias"])
    post = postnet(p, conf, before, flens) if conf.get("postnet_layers", 5) > 0 else None
    after, dn = finish(before, post, flens, mean, std)
    return dict(duration=d, pitch=pitch, energy=energy, hs_embed=hs_e, regulated=reg,
                before=before * _mask(flens, before.shape[1], before), feat_gen=after, feat_gen_denorm=dn, frame_lens=flens)


def ragged_text(p, conf, ids, lens, spembs, style, dtype):
    """The text side (fs2_ragged_ref.ragged_forward's computation, with the style embedding [1][d] of a GST model added in
    front of the x-vector integration): (hs [B][T][d], logd [B][T])."""
    B, T = ids.shape
    c = RR.oracle_config(conf, p["encoder.embed.0.weight"].shape[0])
    x = F.embedding(ids, p["encoder.embed.0.weight"]) * math.sqrt(c.adim)
    hs = conformer_stack(p, "encoder", c.enc_blocks, c, c.enc_kernel, x, lens)
    if style is not None:
        hs = hs + style.to(dtype)[:, None]
    if spembs is not None:      # fastspeech2.py:784-808
        s = F.normalize(torch.as_tensor(np.asarray(spembs)).to(hs.device, dtype)[None])
        if conf.get("spk_embed_integration_type", "add") == "add":
            hs = hs + F.linear(s, p["projection.weight"], p["projection.bias"])[:, None]
        else:
            hs = F.linear(torch.cat([hs, s[:, None].expand(B, T, -1)], dim=-1), p["projection.weight"], p["projection.bias"])
    mask = _mask(lens, T, hs)
    y = (hs * mask).transpose(1, 2)
    n_layers = conf.get("duration_predictor_layers", 2)
    pad = (conf.get("duration_predictor_kernel_size", 3) - 1) // 2
    for l in range(n_layers):
        pre = f"duration_predictor.conv.{l}."
        y = torch.relu(F.conv1d(y, p[pre + "0.weight"], p[pre + "0.bias"], padding=pad))
        y = F.layer_norm(y.transpose(1, 2), (y.shape[1],), p[pre + "2.weight"], p[pre + "2.bias"], 1e-12)
        y = (y * mask if l < n_layers - 1 else y).transpose(1, 2)
    logd = F.linear(y.transpose(1, 2), p["duration_predictor.linear.weight"], p["duration_predictor.linear.bias"]).squeeze(-1)
    return hs, logd
