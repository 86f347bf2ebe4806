"""CPU yardsticks of the batched editor's rows="alone": every row of a ragged batch computed as the reference's B = 1 driver
computes that request alone.  Built from the oracle's own functions (collate, model_forward and the blocks) and the existing
ragged restatements of tests/fs2_ragged_ref.py.

  * oracle_rows_alone: per request the oracle's collate and eval-mode forward of THAT request alone -- the reference.
  * packed_forward: the rule the device path follows, stated on a padded batch:
      1. the pre-speech blocks run over the speech tokens at T = T_mel with per-row lengths sl_b;
      2. the rows are packed: row b = its sl_b speech tokens, its tl_b text tokens directly behind them, zeros;
      3. the encoder's positional rows are cat(pe[:sl_b], pe[:tl_b]) per row, the decoder's pe[:n_b], n_b = sl_b + tl_b;
      4. keys j >= n_b are masked and the legacy rel_shift is taken on the n_b x n_b block of the compact position scores;
      5. every convolution with more than one tap reads zeros behind the row's length: both FFN convs, the depthwise conv,
         and in the postnet its input and the output of every BatchNorm'ed layer (zeroed behind sl_b);
      6. everything else is row-wise.
Not a test module: tests/test_sedit_rows_alone_host.py and tests/test_gpu_sedit_rows_alone.py import it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import fs2_ragged_ref as RR
import mlm_variants_ref as V
import test_gpu_sedit_batch as SB      # the fixture: _requests, _ids, _opts (its module imports need no device)
from oracle import a3t_oracle as O

SPAN_GAP = 0.1          # rows 0 and 1 of the fixture batch miss the row alone by at least this inside their spans
MEL_BOUND = 1e-3        # atol = rtol of test_inference_batch_against_oracle, the device test's bound
RULE_BOUND = 1e-5       # of scale: the packed-row rule against the row alone, fp32 on the CPU


def plan_data(reqs, oc, dur):
    """Per request the oracle's plan: ([(uid, collate dict)], [(old span, new span)])."""
    data, plans = [], []
    ids = SB._ids(oc)
    for i, r in enumerate(reqs):
        ms, me, op, nph, rep, add = O.sedit_phone_spans(r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str)
        nwav, phns, ns, ne, ob, nb = O.sedit_plan_edit(r.wav_org, oc.fs, oc.hop_length, ms, me, op, nph, rep, add, dur, r.new_str,
                                                       **SB._opts(r))
        plans.append((ob, nb))
        data.append((str(i), dict(speech=np.asarray(nwav, np.float32), align_start=np.asarray(ns), align_end=np.asarray(ne),
                                  text=ids(phns), span_boundary=np.asarray(nb))))
    return data, plans


def fake_duration():
    """The duration stand-in of the existing editor tests (tests/golden/make_golden.py)."""
    import sys
    if SB.G not in sys.path:
        sys.path.insert(0, SB.G)
    from make_golden import fake_phone_duration
    return fake_phone_duration


_CACHE = {}


def oracle_rows_alone(seed=SB.MODEL_SEED):
    """The four fixture requests, each collated and run ALONE by the oracle (eval mode).  Computed once per seed and shared:
    dict(data, plans, batches [per row the B = 1 collate], after [per row (T_b, odim)], rows [per row the spliced mel])."""
    if seed in _CACHE:
        return _CACHE[seed]
    oc = O.tiny_config()
    state = O.to_torch_state(O.procedural_state(O.param_shapes(oc), seed))
    data, plans = plan_data(SB._requests(), oc, fake_duration())
    batches, afters, rows = [], [], []
    for d, (ob, nb) in zip(data, plans):
        b = O.collate([d], oc)[1]
        with torch.no_grad():
            _, after = O.model_forward(state, b, oc, train_bn=False)
        s, e = nb
        batches.append(b)
        afters.append(after[0])
        rows.append(torch.cat([b["speech"][0, :s], after[0, s:e], b["speech"][0, e:]], dim=0))
    _CACHE[seed] = dict(oc=oc, state=state, data=data, plans=plans, batches=batches, after=afters, rows=rows)
    return _CACHE[seed]


def alone_collated_batch(ref):
    """The padded batch whose row b holds the B = 1 collate of request b: what MLMCollateFn(rows="alone") returns.  The integer
    outputs are the batch collate's (they are row-local), the mels the rows' own."""
    oc = ref["oc"]
    b = O.collate(ref["data"], oc)[1]
    speech = torch.zeros_like(b["speech"])
    for i, one in enumerate(ref["batches"]):
        n = one["speech"].shape[1]
        speech[i, :n] = one["speech"][0]
        for k in ("masked_position", "speech_mask", "text_mask", "speech_segment_pos", "text_segment_pos", "text"):
            w = one[k].shape[-1]
            assert torch.equal(b[k][i][..., :w], one[k][0]) and not b[k][i][..., w:].any(), (k, i)
    return dict(b, speech=speech)


def short_batch(c, seed=7):
    """Rows (T_mel, T_phn) = (40, 3), (9, 8), (2, 1) in one padded batch; the last is shorter than every depthwise kernel."""
    sl, tl = [40, 9, 2], [3, 8, 1]
    return O.synthetic_batch(c, B=3, T_mel=40, T_phn=8, seed=seed, lengths=sl, text_lengths=tl), sl, tl


def row_alone(batch, b, sl, tl):
    """Row b of a padded batch as a batch of its own at its exact lengths."""
    cut = {"speech": sl, "masked_position": sl, "speech_mask": sl, "speech_segment_pos": sl, "text": tl, "text_mask": tl,
           "text_segment_pos": tl}
    out = {}
    for k, v in batch.items():
        if k not in cut:
            out[k] = v[b:b + 1]
        elif k == "speech":
            out[k] = v[b:b + 1, :sl]
        else:
            out[k] = v[b:b + 1, ..., :cut[k]]
    return out


def _attention_rows(x, pos, lens, p, pre, c):
    """fs2_ragged_ref._attention with positional rows of its own per batch row: pos [B][T][d]."""
    B, T, d = x.shape
    H, dk = c.heads, c.dk
    q = F.linear(x, p[pre + "linear_q.weight"], p[pre + "linear_q.bias"]).view(B, T, H, dk)
    k = F.linear(x, p[pre + "linear_k.weight"], p[pre + "linear_k.bias"]).view(B, T, H, dk).transpose(1, 2)
    v = F.linear(x, p[pre + "linear_v.weight"], p[pre + "linear_v.bias"]).view(B, T, H, dk).transpose(1, 2)
    pp = F.linear(pos, p[pre + "linear_pos.weight"]).view(B, T, H, dk).transpose(1, 2)
    ac = torch.matmul((q + p[pre + "pos_bias_u"]).transpose(1, 2), k.transpose(-2, -1))
    bd = torch.matmul((q + p[pre + "pos_bias_v"]).transpose(1, 2), pp.transpose(-2, -1))
    attn = RR.ragged_softmax(ac, bd, lens, 1.0 / math.sqrt(dk))
    ctx = torch.matmul(attn, v).transpose(1, 2).contiguous().view(B, T, d)
    return F.linear(ctx, p[pre + "linear_out.weight"], p[pre + "linear_out.bias"])


def _block(x, pos, lens, p, pre, c, K):
    mask = RR._row_mask(lens, x.shape[1], x.dtype)
    x = x + 0.5 * RR._ffn(O._ln(x, p, pre + "norm_ff_macaron", 1e-12), mask, p, pre + "feed_forward_macaron.", c)
    x = x + _attention_rows(O._ln(x, p, pre + "norm_mha", 1e-12), pos, lens, p, pre + "self_attn.", c)
    x = x + RR._conv_module(O._ln(x, p, pre + "norm_conv", 1e-12), mask, p, pre + "conv_module.", K)
    x = x + 0.5 * RR._ffn(O._ln(x, p, pre + "norm_ff", 1e-12), mask, p, pre + "feed_forward.", c)
    return O._ln(x, p, pre + "norm_final", 1e-12)


def packed_forward(p, batch, c, slens, tlens, segment_emb=True, pre_blocks=0, has_decoder=True):
    """The packed-row rule (module docstring) on a padded batch, eval mode.  Returns before, after [B][T_mel][odim]; rows behind
    slens[b] mean nothing.  The speech and text masks of the batch are not read."""
    dt = p["sfc.weight"].dtype
    speech = batch["speech"].to(dt)
    B, Tm, _ = speech.shape
    d = c.adim
    mpos = batch["masked_position"].bool()[..., None]
    x = speech.masked_fill(mpos, 0) + p["encoder.speech_embed.0.mask_feature"].expand_as(speech).masked_fill(~mpos, 0)
    x = F.linear(x, p["encoder.speech_embed.1.weight"], p["encoder.speech_embed.1.bias"])
    x = F.layer_norm(x, (d,), p["encoder.speech_embed.2.weight"], p["encoder.speech_embed.2.bias"], 1e-5)
    x = torch.relu(x) * math.sqrt(d)
    text = batch["text"]
    Tp = text.shape[1]
    T = Tm + Tp
    Vn = p["encoder.text_embed.0.weight"].shape[0]
    xt = F.embedding(text, p["encoder.text_embed.0.weight"], padding_idx=Vn - 1) * math.sqrt(d)
    if segment_emb:
        seg = p["encoder.segment_emb.weight"]
        x = x + F.embedding(batch["speech_segment_pos"], seg, padding_idx=c.seg_table - 1)
        xt = xt + F.embedding(batch["text_segment_pos"], seg, padding_idx=c.seg_table - 1)
    if "spk_proj.weight" in p and batch.get("spembs") is not None:
        s = F.linear(batch["spembs"].to(dt), p["spk_proj.weight"], p["spk_proj.bias"])[:, None]
        x, xt = x + s, xt + s
    pe = O.legacy_pe(c, T, dt)
    for i in range(pre_blocks):
        x = _block(x, pe[:Tm][None].expand(B, Tm, d), slens, p, f"encoder.pre_speech_encoders.{i}.", c, c.enc_kernel)
    xs, pos = x.new_zeros(B, T, d), x.new_zeros(B, T, d)
    n = [s + t for s, t in zip(slens, tlens)]
    for b, (s, t) in enumerate(zip(slens, tlens)):
        xs[b, :s], xs[b, s:s + t] = x[b, :s], xt[b, :t]
        pos[b, :s], pos[b, s:s + t] = pe[:s], pe[:t]
    for i in range(c.enc_blocks):
        xs = _block(xs, pos, n, p, f"encoder.encoders.{i}.", c, c.enc_kernel)
    xs = O._ln(xs, p, "encoder.after_norm", 1e-12)
    if has_decoder:
        xs = xs * math.sqrt(d)
        for i in range(c.dec_blocks):
            xs = _block(xs, pe[None].expand(B, T, d), n, p, f"decoder.encoders.{i}.", c, c.dec_kernel)
        xs = O._ln(xs, p, "decoder.after_norm", 1e-12)
    before = F.linear(xs[:, :Tm].contiguous(), p["sfc.weight"], p["sfc.bias"])
    if c.postnet_layers == 0:
        return before, None
    smask = RR._row_mask(slens, Tm, dt)
    y = (before * smask).transpose(1, 2)
    for l in range(c.postnet_layers):
        pre = f"postnet.postnet.{l}."
        y = F.conv1d(y, p[pre + "0.weight"], None, padding=(c.postnet_filts - 1) // 2)
        y = O._batch_norm(y, p, pre + "1", False)
        if l != c.postnet_layers - 1:
            y = torch.tanh(y)
        y = y * smask.transpose(1, 2)
    return before, before * smask + y.transpose(1, 2)


def of_scale(got, ref):
    """max |got - ref| relative to the reference's scale max(1, max |ref|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max())) if ref.size else 0.0
