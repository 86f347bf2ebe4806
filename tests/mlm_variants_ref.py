"""CPU restatement of the masked-mel model's forward for the variants MLMTask builds besides the recipe's: no segment
embedding (input_layer 'mlm'), pre-speech blocks (pre_speech_layer N) and no_decoder.  Built from oracle.a3t_oracle's own
functions (conformer_block, _ln, legacy_pe, mlm_loss and the postnet part of model_forward); fp32 or fp64 by the dtype of
the state.  tests/golden/mlm_variants.npz pins it against the reference.
"""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import a3t_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# case -> (segment_emb, pre_blocks, has_decoder), the options tests/golden/make_golden_mlm_variants.py passed the reference
CASES = {"a": (False, 0, True), "b": (True, 2, True), "c": (True, 0, False), "d": (False, 1, False)}
SEED_W, SEED_B = 1, 11


def load_golden(case):
    """The reference's records of one case: scalars / outputs / buffers and the gradients, with the case prefix stripped."""
    out = {}
    for f in ("mlm_variants.npz", f"mlm_variants_grads_{case}.npz"):
        z = np.load(os.path.join(GOLD, f))
        out.update({k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + ".")})
    return out


def golden_keys(case):
    """{reference state-dict key: shape} of one case."""
    meta = json.load(open(os.path.join(GOLD, "mlm_variants.json")))
    return {k: tuple(s) for k, s in meta["cases"][case]["keys"].items()}


def tiny_batch(case):
    c = O.tiny_config()
    b = O.synthetic_batch(c, B=2, T_mel=48, T_phn=8, seed=SEED_B, lengths=[48, 37], text_lengths=[8, 6])
    if not CASES[case][0]:        # the reference's collate returns all-zero segment ids for input_layer 'mlm'
        b["speech_segment_pos"] = torch.zeros_like(b["speech_segment_pos"])
        b["text_segment_pos"] = torch.zeros_like(b["text_segment_pos"])
    return c, b


def procedural(case, dtype=torch.float32, requires_grad=False):
    return O.to_torch_state(O.procedural_state(golden_keys(case), seed=SEED_W), dtype, requires_grad)


def variant_forward(p, batch, c, segment_emb=True, pre_blocks=0, has_decoder=True, train_bn=True, stats_out=None):
    """ESPnetMLMEncAsDecoderModel._forward for the variant (conformer/encoder.py:522-566, sedit_model.py:350-375).
    Returns before, after."""
    speech = batch["speech"]
    dt = p["sfc.weight"].dtype
    speech = speech.to(dt)
    B, Tm, _ = speech.shape
    d = c.adim
    mpos = batch["masked_position"].bool()[..., None]
    x = speech.masked_fill(mpos, 0) + p["encoder.speech_embed.0.mask_feature"].expand_as(speech).masked_fill(~mpos, 0)
    x = F.linear(x, p["encoder.speech_embed.1.weight"], p["encoder.speech_embed.1.bias"])
    x = F.layer_norm(x, (d,), p["encoder.speech_embed.2.weight"], p["encoder.speech_embed.2.bias"], 1e-5)
    x = torch.relu(x) * math.sqrt(d)
    text = batch["text"]
    Tp = text.shape[1]
    V = p["encoder.text_embed.0.weight"].shape[0]
    xt = F.embedding(text, p["encoder.text_embed.0.weight"], padding_idx=V - 1) * math.sqrt(d)
    if segment_emb:       # (without the table the segment ids are not looked at, conformer/encoder.py:541)
        seg = p["encoder.segment_emb.weight"]
        x = x + F.embedding(batch["speech_segment_pos"], seg, padding_idx=c.seg_table - 1)
        xt = xt + F.embedding(batch["text_segment_pos"], seg, padding_idx=c.seg_table - 1)
    if "spk_proj.weight" in p and batch.get("spembs") is not None:
        # x-vector conditioning (a local extension, no reference behaviour): Linear(spembs) added to every token at the
        # prologue, so the pre-speech blocks see it
        s = F.linear(batch["spembs"].to(dt), p["spk_proj.weight"], p["spk_proj.bias"])[:, None]
        x, xt = x + s, xt + s
    pos_s = O.legacy_pe(c, Tm, dt)[None]
    for i in range(pre_blocks):      # the speech tokens alone: T = T_mel, speech_mask, pe[:T_mel]
        x = O.conformer_block(x, pos_s, batch["speech_mask"], p, f"encoder.pre_speech_encoders.{i}.", c, c.enc_kernel,
                              train_bn, stats_out)
    xs = torch.cat([x, xt], dim=1)
    pos = torch.cat([pos_s, O.legacy_pe(c, Tp, dt)[None]], dim=1)
    masks = torch.cat([batch["speech_mask"], batch["text_mask"]], dim=-1)
    for i in range(c.enc_blocks):
        xs = O.conformer_block(xs, pos, masks, p, f"encoder.encoders.{i}.", c, c.enc_kernel, train_bn, stats_out)
    xs = O._ln(xs, p, "encoder.after_norm", 1e-12)
    if has_decoder:
        T = xs.shape[1]
        xs = xs * math.sqrt(d)
        posd = O.legacy_pe(c, T, dt)[None]
        for i in range(c.dec_blocks):
            xs = O.conformer_block(xs, posd, masks, p, f"decoder.encoders.{i}.", c, c.dec_kernel, train_bn, stats_out)
        xs = O._ln(xs, p, "decoder.after_norm", 1e-12)
    before = F.linear(xs[:, :Tm].contiguous(), p["sfc.weight"], p["sfc.bias"])
    if c.postnet_layers == 0:
        return before, None
    y = before.transpose(1, 2)
    for l in range(c.postnet_layers):
        pre = f"postnet.postnet.{l}."
        y = F.conv1d(y, p[pre + "0.weight"], None, padding=(c.postnet_filts - 1) // 2)
        y = O._batch_norm(y, p, pre + "1", train_bn, stats_out)
        if l != c.postnet_layers - 1:
            y = torch.tanh(y)
    return before, before + y.transpose(1, 2)


def variant_loss(p, batch, c, case, train_bn=True, stats_out=None):
    seg, pre, dec = CASES[case]
    before, after = variant_forward(p, batch, c, seg, pre, dec, train_bn, stats_out)
    loss = O.mlm_loss(before, after, batch["speech"].to(before.dtype), batch["masked_position"], c)
    return loss, before, after


def variant_splice(p, batch, c, case, span):
    seg, pre, dec = CASES[case]
    _, after = variant_forward(p, batch, c, seg, pre, dec, train_bn=False)
    s, e = span
    return torch.cat([batch["speech"][0, :s].to(after.dtype), after[0, s:e], batch["speech"][0, e:].to(after.dtype)], dim=0)
