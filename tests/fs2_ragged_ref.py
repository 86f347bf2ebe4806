"""CPU restatement of the FastSpeech2 duration path over a padded batch with per-row lengths ("ragged" semantics): the
yardstick of the batched duration model (a3t_amd/duration.py::forward_ids_batch), built from the oracle's blocks.

Row b of a padded [B][Tmax] batch must get what it would get alone at n = lens[b]:
  1. attention: keys j >= n are masked and the legacy rel_shift is taken on the n x n block of the compact (q + v) P^T
     matrix (P = linear_pos(pe[:Tmax]): its first n rows are pe[:n] projected, what the row alone uses);
  2. every convolution with more than one tap reads zeros behind n: the LayerNorm output in front of the first FFN conv,
     the hidden tensor between the two FFN convs, the GLU output in front of the depthwise conv, the input of the first
     duration-predictor conv and the LayerNorm output between predictor convs;
  3. everything else is row-wise; rows behind n hold anything finite.
Not a test module: tests/test_duration_batch_host.py and tests/test_gpu_duration_batch.py import it."""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from oracle import a3t_oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def meta():
    return json.load(open(os.path.join(G, "fs2_duration.json")))


def arrays():
    return np.load(os.path.join(G, "fs2_duration.npz"))


def checkpoint(m, case):
    """(ESPnet config dict, state dict under the FastSpeech2 names without 'tts.') of a fixture model, overrides applied."""
    mc = m["cases"][case]
    state = O.procedural_state({k: tuple(v) for k, v in mc["shapes"].items()}, mc["seed"])
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden_fs2 import apply_overrides      # the fixture's documented overrides (imports nothing of the reference)
    apply_overrides(state, mc["tts_conf"].get("duration_predictor_layers", 2))
    cfg = {"tts": "fastspeech2", "tts_conf": mc["tts_conf"], "token_list": m["token_list"]}
    return cfg, {k: torch.from_numpy(np.array(v)) for k, v in state.items()}


def tie_distance(e):
    """Distance of e to the nearest k + 0.5."""
    e = np.asarray(e, np.float64)
    return np.abs(e - np.floor(e) - 0.5)


def fixture_batch(z, m, case, pad_ids=None):
    """The fixture's lengths of one model as ONE padded batch: (ids [B][Tmax] int64, lens list).  pad_ids: a RandomState to
    draw valid ids for the padding from; None pads with 0."""
    lens = list(m["lengths"])
    Tmax = max(lens)
    ids = np.zeros((len(lens), Tmax), np.int64)
    if pad_ids is not None:
        ids[:] = pad_ids.randint(0, len(m["token_list"]), size=ids.shape)
    for b, T in enumerate(lens):
        ids[b, :T] = z[f"{case}.T{T}.ids"]
    return ids, lens


def _row_mask(lens, T, dtype):
    """[B][T][1]: 1 for t < lens[b]."""
    return (torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]).to(dtype).unsqueeze(-1)


def ragged_softmax(ac, bd, lens, scale):
    """probs [B][H][T][T] from content scores ac and the COMPACT position scores bd of the padded launch: per row b softmax over
    the n x n block with rel_shift_legacy taken on that block; 0 for keys and query rows >= n."""
    out = torch.zeros_like(ac)
    for b, n in enumerate(lens):
        s = (ac[b:b + 1, :, :n, :n] + O.rel_shift_legacy(bd[b:b + 1, :, :n, :n].contiguous())) * scale
        out[b, :, :n, :n] = torch.softmax(s, dim=-1)[0]
    return out


def _attention(x, pos, lens, p, pre, c):
    B, T, d = x.shape
    H, dk = c.heads, c.dk
    q = F.linear(x, p[pre + "linear_q.weight"], p[pre + "linear_q.bias"]).view(B, T, H, dk)
    k = F.linear(x, p[pre + "linear_k.weight"], p[pre + "linear_k.bias"]).view(B, T, H, dk).transpose(1, 2)
    v = F.linear(x, p[pre + "linear_v.weight"], p[pre + "linear_v.bias"]).view(B, T, H, dk).transpose(1, 2)
    pp = F.linear(pos, p[pre + "linear_pos.weight"]).view(1, -1, H, dk).transpose(1, 2)
    ac = torch.matmul((q + p[pre + "pos_bias_u"]).transpose(1, 2), k.transpose(-2, -1))
    bd = torch.matmul((q + p[pre + "pos_bias_v"]).transpose(1, 2), pp.transpose(-2, -1))
    attn = ragged_softmax(ac, bd, lens, 1.0 / math.sqrt(dk))
    ctx = torch.matmul(attn, v).transpose(1, 2).contiguous().view(B, T, d)
    return F.linear(ctx, p[pre + "linear_out.weight"], p[pre + "linear_out.bias"])


def _ffn(x, mask, p, pre, c):
    """ffn_conv of the oracle with zeros behind every row's length in front of both convs (x is the LayerNorm output)."""
    pad = (c.ff_kernel - 1) // 2
    h = torch.relu(F.conv1d((x * mask).transpose(1, 2), p[pre + "w_1.weight"], p[pre + "w_1.bias"], padding=pad))
    h = h * mask.transpose(1, 2)
    return F.conv1d(h, p[pre + "w_2.weight"], p[pre + "w_2.bias"], padding=pad).transpose(1, 2)


def _conv_module(x, mask, p, pre, K):
    y = F.conv1d(x.transpose(1, 2), p[pre + "pointwise_conv1.weight"], p[pre + "pointwise_conv1.bias"])
    y = F.glu(y, dim=1) * mask.transpose(1, 2)
    y = F.conv1d(y, p[pre + "depthwise_conv.weight"], p[pre + "depthwise_conv.bias"], padding=(K - 1) // 2, groups=y.shape[1])
    y = O._batch_norm(y, p, pre + "norm", False)
    y = y * torch.sigmoid(y)
    return F.conv1d(y, p[pre + "pointwise_conv2.weight"], p[pre + "pointwise_conv2.bias"]).transpose(1, 2)


def oracle_config(conf, vocab):
    return O.A3TConfig(vocab=vocab, adim=conf["adim"], heads=conf["aheads"], ff=conf["eunits"],
                       ff_kernel=conf["positionwise_conv_kernel_size"], enc_blocks=conf["elayers"],
                       enc_kernel=conf["conformer_enc_kernel_size"])


def ragged_forward(p, conf, ids, lens, spembs=None, dtype=torch.float32, keep=None):
    """p: state dict under the FastSpeech2 names; conf: tts_conf; ids [B][Tmax] int64 (numpy or torch), lens: list of B ints.
    Returns (hs [B][Tmax][d], logd [B][Tmax]) as torch tensors of `dtype`; entries behind lens[b] mean nothing.
    keep (a dict): receives the output of every encoder block as keep["enc.<i>"]."""
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}
    ids = torch.as_tensor(np.asarray(ids))
    B, T = ids.shape
    c = oracle_config(conf, p["encoder.embed.0.weight"].shape[0])
    mask = _row_mask(lens, T, dtype)
    x = F.embedding(ids, p["encoder.embed.0.weight"]) * math.sqrt(c.adim)
    pos = O.legacy_pe(c, T, dtype)[None]
    for i in range(c.enc_blocks):
        pre = f"encoder.encoders.{i}."
        x = x + 0.5 * _ffn(O._ln(x, p, pre + "norm_ff_macaron", 1e-12), mask, p, pre + "feed_forward_macaron.", c)
        x = x + _attention(O._ln(x, p, pre + "norm_mha", 1e-12), pos, lens, p, pre + "self_attn.", c)
        x = x + _conv_module(O._ln(x, p, pre + "norm_conv", 1e-12), mask, p, pre + "conv_module.", c.enc_kernel)
        x = x + 0.5 * _ffn(O._ln(x, p, pre + "norm_ff", 1e-12), mask, p, pre + "feed_forward.", c)
        x = O._ln(x, p, pre + "norm_final", 1e-12)
        if keep is not None:
            keep[f"enc.{i}"] = x
    hs = O._ln(x, p, "encoder.after_norm", 1e-12)
    if spembs is not None:      # fastspeech2.py:784-808
        s = F.normalize(torch.as_tensor(np.asarray(spembs)).to(dtype)[None])
        if conf.get("spk_embed_integration_type", "add") == "add":
            hs = hs + F.linear(s, p["projection.weight"], p["projection.bias"])[:, None]
        else:
            hs = F.linear(torch.cat([hs, s[:, None].expand(B, T, -1)], dim=-1), p["projection.weight"], p["projection.bias"])
    y = (hs * mask).transpose(1, 2)
    n_layers = conf.get("duration_predictor_layers", 2)
    pad = (conf.get("duration_predictor_kernel_size", 3) - 1) // 2
    for l in range(n_layers):      # duration_predictor.py: Conv1d, ReLU, LayerNorm over channels, dropout
        pre = f"duration_predictor.conv.{l}."
        y = torch.relu(F.conv1d(y, p[pre + "0.weight"], p[pre + "0.bias"], padding=pad))
        y = F.layer_norm(y.transpose(1, 2), (y.shape[1],), p[pre + "2.weight"], p[pre + "2.bias"], 1e-12)
        y = (y * mask if l < n_layers - 1 else y).transpose(1, 2)
    logd = F.linear(y.transpose(1, 2), p["duration_predictor.linear.weight"], p["duration_predictor.linear.bias"]).squeeze(-1)
    return hs, logd


def frames_of(logd, offset=1.0):
    return torch.clamp(torch.round(torch.exp(logd) - offset), min=0).long()
