"""CPU restatement of the masked-mel model with `encoder: transformer` (MLMEncoder / MLMDecoder of transformer/encoder.py:370-777):
pre-LN blocks of plain MultiHeadedAttention and a position-wise FFN (`linear`, or conv1d with k taps), absolute positions added
where speech_embed / text_embed end and at the decoder entry (PositionalEncoding, or ScaledPositionalEncoding with its two
alphas).  Plain torch, fp32 or fp64 by the dtype of the state; the head, postnet and loss are oracle.a3t_oracle's.
tests/golden/mlm_transformer*.npz pins it against the reference, each output within the reference's own fp32-against-fp64
distance (tolerance()).
"""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import a3t_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLD, "mlm_transformer.json")))
CASES = sorted(META["cases"])
SEED_W, SEED_B = META["seed_weights"], META["seed_batch"]
ALPHAS = META["alphas"]


def options(case):
    return META["cases"][case]["options"]


def load_golden(case):
    """The reference's records of one case (outputs, `err.<output>` distances, gradients), the case prefix stripped."""
    out = {}
    for f in ("mlm_transformer.npz", f"mlm_transformer_grads_{case}.npz"):
        z = np.load(os.path.join(GOLD, f))
        out.update({k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + ".")})
    return out


def golden_keys(case):
    return {k: tuple(s) for k, s in META["cases"][case]["keys"].items()}


def tolerance(g, name):
    """Absolute bound on |x - reference fp32| for the output `name` of a computation that carries fp32 rounding of its own.
    err = max |reference fp32 - reference fp64| is what one fp32 evaluation in the reference's order is off by; another order of
    the same sums is off by as much in its own direction, so two evaluations differ by up to 2 err, and err is one draw of that
    distance, not its maximum: 4 err.  For a tensor err is the largest of many draws; for a scalar (the loss, an alpha gradient) it is
    a single one and can land near zero by chance (the text alpha's gradient of case b: 3.5e-8 on a value of 1.4, a quarter of an
    ulp, where the speech alpha's is 2.5e-6 on 9).  So err is never taken below the case's typical distance: the median over all of the
    case's recorded outputs of err / largest magnitude, times this output's largest magnitude."""
    def scale(n):
        return max(float(np.abs(np.asarray(g[n], dtype=np.float64)).max()), 1e-30)
    names = [k[4:] for k in g if k.startswith("err.")]
    typical = float(np.median([float(g["err." + n]) / scale(n) for n in names]))
    return 4.0 * max(float(g["err." + name]), typical * scale(name))


def tiny_batch(case):
    c = O.tiny_config()
    b = O.synthetic_batch(c, B=2, T_mel=48, T_phn=8, seed=SEED_B, lengths=[48, 37], text_lengths=[8, 6])
    if options(case)["input_layer"] == "mlm":        # the reference's collate returns all-zero segment ids for input_layer 'mlm'
        b["speech_segment_pos"] = torch.zeros_like(b["speech_segment_pos"])
        b["text_segment_pos"] = torch.zeros_like(b["text_segment_pos"])
    return c, b


def procedural(case, dtype=torch.float32, requires_grad=False):
    state = O.procedural_state(golden_keys(case), seed=SEED_W)
    for k, a in ALPHAS.items():
        if k in state:
            state[k] = np.array(a, dtype=np.float32)
    return O.to_torch_state(state, dtype, requires_grad)


def abs_pe(c, T, dtype=torch.float32):
    """PositionalEncoding.pe rows 0..T-1 (transformer/embedding.py:59-80, reverse=False), computed in fp32 as the reference does."""
    d = c.adim
    position = torch.arange(0, T, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe = torch.zeros(T, d)
    pe[:, 0::2] = torch.sin(position * div)
    pe[:, 1::2] = torch.cos(position * div)
    return pe.to(dtype)


def plain_attention(x, mask, p, pre, c, return_probs=False):
    """MultiHeadedAttention.forward (attention.py:98-122, forward_qkv :40-62, forward_attention :64-96).  mask: B*T booleans."""
    B, T, d = x.shape
    H, dk = c.heads, c.dk
    q = F.linear(x, p[pre + "linear_q.weight"], p[pre + "linear_q.bias"]).view(B, T, H, dk).transpose(1, 2)
    k = F.linear(x, p[pre + "linear_k.weight"], p[pre + "linear_k.bias"]).view(B, T, H, dk).transpose(1, 2)
    v = F.linear(x, p[pre + "linear_v.weight"], p[pre + "linear_v.bias"]).view(B, T, H, dk).transpose(1, 2)
    scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(dk)
    dead = ~mask.reshape(B, 1, 1, T).bool()
    scores = scores.masked_fill(dead, torch.finfo(scores.dtype).min)
    probs = torch.softmax(scores, dim=-1).masked_fill(dead, 0.0)
    ctx = torch.matmul(probs, v).transpose(1, 2).contiguous().view(B, T, d)
    out = F.linear(ctx, p[pre + "linear_out.weight"], p[pre + "linear_out.bias"])
    return (out, probs) if return_probs else out


def ffn(x, p, pre):
    """PositionwiseFeedForward (w_1.weight [ff][d]) or MultiLayeredConv1d (w_1.weight [ff][d][k]), told apart by the weight."""
    w1, w2 = p[pre + "w_1.weight"], p[pre + "w_2.weight"]
    if w1.dim() == 2:
        return F.linear(torch.relu(F.linear(x, w1, p[pre + "w_1.bias"])), w2, p[pre + "w_2.bias"])
    pad = (w1.shape[2] - 1) // 2
    h = torch.relu(F.conv1d(x.transpose(1, 2), w1, p[pre + "w_1.bias"], padding=pad))
    return F.conv1d(h, w2, p[pre + "w_2.bias"], padding=pad).transpose(1, 2)


def transformer_block(x, mask, p, pre, c):
    """EncoderLayer.forward (transformer/encoder_layer.py:62-121): normalize_before, no concat_after, dropout 0."""
    x = x + plain_attention(O._ln(x, p, pre + "norm1", 1e-12), mask, p, pre + "self_attn.", c)
    return x + ffn(O._ln(x, p, pre + "norm2", 1e-12), p, pre + "feed_forward.")


def prologue(p, batch, c):
    """speech_embed / text_embed with their positional encodings, then the segment embedding (transformer/encoder.py:705-721)."""
    dt = p["sfc.weight"].dtype
    speech = batch["speech"].to(dt)
    B, Tm, _ = speech.shape
    d = c.adim
    mpos = batch["masked_position"].bool()[..., None]
    x = speech.masked_fill(mpos, 0) + p["encoder.speech_embed.0.mask_feature"].expand_as(speech).masked_fill(~mpos, 0)
    x = F.linear(x, p["encoder.speech_embed.1.weight"], p["encoder.speech_embed.1.bias"])
    x = torch.relu(F.layer_norm(x, (d,), p["encoder.speech_embed.2.weight"], p["encoder.speech_embed.2.bias"], 1e-5))
    text = batch["text"]
    Tp = text.shape[1]
    V = p["encoder.text_embed.0.weight"].shape[0]
    xt = F.embedding(text, p["encoder.text_embed.0.weight"], padding_idx=V - 1)
    if "encoder.speech_embed.4.alpha" in p:      # ScaledPositionalEncoding (embedding.py:143-147)
        x = x + p["encoder.speech_embed.4.alpha"] * abs_pe(c, Tm, dt)
        xt = xt + p["encoder.text_embed.1.alpha"] * abs_pe(c, Tp, dt)
    else:                                        # PositionalEncoding (embedding.py:82-85)
        x = x * math.sqrt(d) + abs_pe(c, Tm, dt)
        xt = xt * math.sqrt(d) + abs_pe(c, Tp, dt)
    if "encoder.segment_emb.weight" in p:
        seg = p["encoder.segment_emb.weight"]
        x = x + F.embedding(batch["speech_segment_pos"], seg, padding_idx=c.seg_table - 1)
        xt = xt + F.embedding(batch["text_segment_pos"], seg, padding_idx=c.seg_table - 1)
    return x, xt


def model_forward(p, batch, c, train_bn=True):
    """ESPnetMLMEncAsDecoderModel._forward (sedit_model.py:350-375) on a transformer encoder / decoder.  Returns before, after."""
    d = c.adim
    x, xt = prologue(p, batch, c)
    Tm = x.shape[1]
    xs = torch.cat([x, xt], dim=1)
    B, T, _ = xs.shape
    masks = torch.cat([batch["speech_mask"].reshape(B, Tm), batch["text_mask"].reshape(B, T - Tm)], dim=-1)
    n = 0
    while f"encoder.encoders.{n}.norm1.weight" in p:
        xs = transformer_block(xs, masks, p, f"encoder.encoders.{n}.", c)
        n += 1
    xs = O._ln(xs, p, "encoder.after_norm", 1e-12)
    if "decoder.after_norm.weight" in p:         # MLMDecoder: embed = PositionalEncoding over the joined row, then its blocks
        xs = xs * math.sqrt(d) + abs_pe(c, T, xs.dtype)
        n = 0
        while f"decoder.encoders.{n}.norm1.weight" in p:
            xs = transformer_block(xs, masks, p, f"decoder.encoders.{n}.", c)
            n += 1
        xs = O._ln(xs, p, "decoder.after_norm", 1e-12)
    before = F.linear(xs[:, :Tm].contiguous(), p["sfc.weight"], p["sfc.bias"])
    if c.postnet_layers == 0:
        return before, None
    y = before.transpose(1, 2)
    for l in range(c.postnet_layers):
        pre = f"postnet.postnet.{l}."
        y = F.conv1d(y, p[pre + "0.weight"], None, padding=(c.postnet_filts - 1) // 2)
        y = O._batch_norm(y, p, pre + "1", train_bn)
        if l != c.postnet_layers - 1:
            y = torch.tanh(y)
    return before, before + y.transpose(1, 2)


def model_loss(p, batch, c, train_bn=True):
    before, after = model_forward(p, batch, c, train_bn)
    loss = O.mlm_loss(before, after, batch["speech"].to(before.dtype), batch["masked_position"], c)
    return loss, before, after


def model_splice(p, batch, c, span):
    _, after = model_forward(p, batch, c, train_bn=False)
    s, e = span
    return torch.cat([batch["speech"][0, :s].to(after.dtype), after[0, s:e], batch["speech"][0, e:].to(after.dtype)], dim=0)
