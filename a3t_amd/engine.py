"""Forward / backward sequencing of the A3T masked-mel training step on one MI355X.

This is the host-side replacement for the autograd graph the reference builds out of
nn.Modules (ESPnetMLMEncAsDecoderModel._forward, espnet2/tts/sedit/sedit_model.py:350-375,
MLMEncoder/MLMDecoder conformer/encoder.py:522-614, EncoderLayer conformer/encoder_layer.py:80-180):
an explicit, allocation-free schedule of liba3t_hip launches on the current HIP stream, with a
hand-derived backward pass.  torch supplies device buffers only.

MLMEngine owns the model AROUND the Conformer blocks -- prologue, encoder / decoder loops, head, loss and the backward
through them -- and nothing inside a block (conformer.py), no stream or event (schedule.py) and no environment variable
(conformer.EngineOptions)."""
import math
from typing import Dict

import torch

from . import ops
from ._lib import ACT_NONE, ACT_TANH, F32
from .conformer import ConformerStack, score_chunks  # noqa: F401  (score_chunks: imported from here by callers)


class MLMEngine(ConformerStack):
    def _begin(self, batch, need_grad):
        """What every forward pass starts with: the shapes, a new step seed, fresh weight shadows, cleared accumulators."""
        speech = batch["speech"].contiguous()
        B, Tm, idim = speech.shape
        text = batch["text"].contiguous()
        Tp = text.shape[1]
        self.dims = (B, Tm, Tp, Tm + Tp)
        self.attn_path, self.block_dims = {}, {}
        self._need_grad = bool(need_grad)
        self._mode_tag = ops.gemm_mode_tag()
        self.step_seed += 1
        self.refresh_weights()
        self._arena_clear("fwd64")
        self._P_ahead, self._pos_ev = {}, None
        return speech.view(B * Tm, idim), text, batch["masked_position"].contiguous().view(torch.uint8)

    def _prologue(self, batch, speech2, text, masked, split):
        """Encoder prologue (conformer/encoder.py:522-553): mask fill, speech embedding Linear + LayerNorm, x-vector Linear,
        token finish.  split: speech and text tokens in buffers of their own (xsp, xst) for the pre-speech blocks or the packed
        rows; otherwise joined along time in xs.  Returns (xs, xsp, xst), the unused ones None."""
        c, p, ws = self.c, self.store.p, self.ws
        B, Tm, Tp, T = self.dims
        d, pp = c.adim, c.positional_dropout_rate
        spos = batch["speech_segment_pos"].contiguous()
        tpos = batch["text_segment_pos"].contiguous()
        xm = self._act("emb.xm", (B * Tm, c.idim))
        ops.mask_fill(speech2, masked, p["mask_feature"], xm)
        e0 = ws.get("emb.e0", (B * Tm, d))
        ops.linear_fwd(xm, self.W("emb.w"), e0, bias=p["emb.b"], compute=self.cmp)
        e = self._ln_fwd("emb.ln", e0, "emb.ln", eps=1e-5, out_dtype=torch.float32)
        xscale = math.sqrt(d)
        seg = p["seg"] if c.segment_emb else None      # (None: the kernels read no segment ids)
        spk = None
        self.sv.pop("spk", None)
        if c.spk_embed_dim > 0 and batch.get("spembs") is not None:
            # x-vector conditioning (configs[3]): Linear(spembs) added to every token of the utterance, fused into the
            # prologue kernel.  fp32 (B x 512 x d: negligible); an extension, the reference ignores spembs
            se = batch["spembs"].to(self.dev, torch.float32).contiguous()
            spk = ws.get("emb.spk", (B, d))
            ops.linear_fwd(se, p["spk.w"], spk, bias=p["spk.b"], compute=F32)
            self.sv["spk"] = se
        self.sv["embed"] = (xm, e, text, spos, tpos, masked, speech2)
        xs = xsp = xst = None
        if self.transformer:     # absolute positions ride on the same pass (a3t_embed_finish_abs_fwd); never split
            xs = ws.get("emb.xs", (B * T, d))
            ops.embed_finish_abs_fwd(e, p["temb"], seg, text, spos, tpos, self.pe_abs, self._alphas(p), xs, B, Tm, Tp, d, xscale,
                                     drop=self._drop(pp, "emb.x") or (0.0, 0), spk=spk)
        elif split:
            xsp, xst = ws.get("emb.xsp", (B * Tm, d)), ws.get("emb.xst", (B * Tp, d))
            ops.embed_finish_fwd(e, p["temb"], seg, text, spos, tpos, xsp, B, Tm, 0, d, xscale,
                                 drop=self._drop(pp, "emb.x") or (0.0, 0), spk=spk)
            ops.embed_finish_fwd(e, p["temb"], seg, text, spos, tpos, xst, B, 0, Tp, d, xscale,
                                 drop=self._drop(pp, "emb.xt") or (0.0, 0), spk=spk)
        else:
            xs = ws.get("emb.xs", (B * T, d))
            ops.embed_finish_fwd(e, p["temb"], seg, text, spos, tpos, xs, B, Tm, Tp, d, xscale,
                                 drop=self._drop(pp, "emb.x") or (0.0, 0), spk=spk)
        return xs, xsp, xst

    def _alphas(self, views):
        """(alpha_s, alpha_t) of ScaledPositionalEncoding as views of the parameter store (store.p) or of its gradients (store.g);
        None with the plain encoding."""
        return (views["emb.alpha_s"], views["emb.alpha_t"]) if self.c.scaled_pos else None

    def _head(self, x, slens=None):
        """Slice the speech frames, sfc, postnet (sedit_model.py:363-372): (hs, before, after), after = None without a postnet
        (the loss then has no after-term, sedit_model.py:333-337, and after_outs = before_outs).  slens (rows alone): the
        postnet's k-tap convolutions read zeros behind slens[b] (a3t_zero_tail on its input and behind every BatchNorm, whose
        shift makes those rows non-zero)."""
        c, p, ws = self.c, self.store.p, self.ws
        B, Tm, _, T = self.dims
        d = c.adim
        hs = self._act("head.hs", (B * Tm, d))
        ops.slice_rows(x, hs, B, T, Tm, d)
        before = ws.get("head.before", (B * Tm, c.odim))
        if self.bf16:
            # the mel projection on the exact-fp32 MFMA from the fp32 LayerNorm output and the fp32 master weights (B*T_mel x 80 x d:
            # ~20 us): `before` is what the postnet amplifies, its last rounding step is the cheapest one to remove
            hs32 = ws.get("head.hs32", (B * Tm, d))
            ops.slice_rows(x, hs32, B, T, Tm, d)
            ops.linear_fwd(hs32, p["sfc.w"], before, bias=p["sfc.b"], compute=F32)
        else:
            ops.linear_fwd(hs, self.W("sfc.w"), before, bias=p["sfc.b"], compute=self.cmp)
        if c.postnet_layers == 0:
            return hs, before, None
        if slens is not None:
            ops.zero_tail(before, slens, 1, B, Tm)
        y, ylo = before, None
        if self.bf16:      # the first conv reads (hi, lo) = (bf16(x), bf16(x - hi)) (EngineOptions.post_f32_first) or bf16(x)
            y = ws.get("head.before16", (B * Tm, c.odim), torch.bfloat16)
            if self.opt.post_f32_first:
                ylo = ws.get("head.before16lo", (B * Tm, c.odim), torch.bfloat16)
                ops.split_bf16(before, y, ylo)
            else:
                ops.cast_bf16(before, y)
        pad = (c.postnet_filts - 1) // 2
        for l in range(c.postnet_layers):
            W = self.W(f"post.{l}.w")
            oc = W.shape[0]
            last = (l == c.postnet_layers - 1)
            z = ws.get(f"post.{l}.z", (B * Tm, oc))
            ops.conv_fwd(y, W, z, Tm, pad, compute=self.cmp)
            if l == 0 and ylo is not None:
                ops.conv_fwd(ylo, W, z, Tm, pad, R=z, compute=self.cmp)        # z += conv(lo)
            o = ws.get(f"post.{l}.o", (B * Tm, oc), torch.float32 if last else self.adt)
            self._bn_fwd(f"post.{l}", z, f"post.{l}.bn", f"post.{l}.bn", ACT_NONE if last else ACT_TANH, o)
            pdr = self._drop(c.postnet_dropout_rate, f"post.{l}")
            if pdr:
                ops.dropout(o, o, *pdr)
            if slens is not None:
                ops.zero_tail(o, slens, 1, B, Tm)
            self.sv[f"post.{l}"] = y
            y = o
        after = ws.get("head.after", (B * Tm, c.odim))
        after.copy_(before)
        ops.axpy(y, after, 1.0)
        return hs, before, after

    def forward(self, batch: Dict[str, torch.Tensor], need_grad: bool = True, gscale: float = 1.0, lens=None):
        """lens = (slens, tlens), device int32 [B]: every row is computed as if it had been passed alone at slens[b] frames and
        tlens[b] phones (_forward_rows_alone; fp32 compute, eval mode, forward only).  No loss is computed then."""
        if lens is not None:
            return self._forward_rows_alone(batch, need_grad, lens)
        c, ws = self.c, self.ws
        (B, Tm, _), Tp, d = batch["speech"].shape, batch["text"].shape[1], c.adim
        T = Tm + Tp
        if self.bf16 and (T % 8 or Tm % 8):
            raise ValueError(f"compute='bf16' needs T_mel and T_mel+T_phn to be multiples of 8, got {Tm}, {T}")
        self._fused_now, self._fused_train_now = main_path = self._attn_choice(B, T, need_grad)
        speech2, text, masked = self._begin(batch, need_grad)
        pp = c.positional_dropout_rate
        keymask = ws.get("keymask", (B, T), torch.uint8)
        keymask[:, :Tm].copy_(batch["speech_mask"].reshape(B, Tm).view(torch.uint8))
        keymask[:, Tm:].copy_(batch["text_mask"].reshape(B, Tp).view(torch.uint8))
        # pre-speech blocks (conformer/encoder.py:547-551): speech and text tokens are finished into buffers of their own, the
        # speech side goes through the pre.{i} blocks at T = T_mel, then the two are joined along time
        xs, xsp, xst = self._prologue(batch, speech2, text, masked, split=c.pre_blocks > 0)
        if self.transformer:     # no relative-position tables, nothing to project ahead
            x = self._encode(xs, B, T, (None, keymask), (None, keymask), self._drop(pp, "dec.x"))
            return self._finish(x, speech2, masked, need_grad, gscale)
        pos_e = self._act("pos.enc", (T, d))
        pos_d = self._act("pos.dec", (T, d))
        pos_on_side = None
        if self._drop(pp, "pos.enc"):      # dropout(pos_emb) (embedding.py:170)
            def drop_pos():
                pf = ws.get("pos.f32", (T, d))
                pf[:Tm].copy_(self.pe[:Tm])
                pf[Tm:].copy_(self.pe[:Tp])
                ops.dropout(pf, pos_e, *self._drop(pp, "pos.enc"))
                pf.copy_(self.pe[:T])
                ops.dropout(pf, pos_d, *self._drop(pp, "pos.dec"))
            if self.side is not None:
                pos_on_side = drop_pos       # only the positional projections (side stream, below) read the dropped tables
            else:
                drop_pos()
            ws.pos_key = None
        elif getattr(ws, "pos_key", None) != (Tm, Tp, pos_e.data_ptr(), pos_d.data_ptr()):
            # (constant for a given (T_mel, T_phn): rebuilt only when the shape or the workspace buffers change)
            pos_e[:Tm].copy_(self.pe[:Tm])
            pos_e[Tm:].copy_(self.pe[:Tp])
            pos_d.copy_(self.pe[:T])
            ws.pos_key = (Tm, Tp, pos_e.data_ptr(), pos_d.data_ptr())     # (on the workspace: engines may share it)
        # linear_pos(pos_emb) of every block (attention.py:188-189) depends on nothing but the table and the weights: all of
        # them are projected up front on the side stream, which is idle in the forward (one stream: inside each block)
        if self.side is not None:
            first = "pre" if c.pre_blocks > 0 else "enc"      # (the dropped tables are made in front of their first reader)

            def project(kind, posx, n):
                def run():
                    if kind == first and pos_on_side is not None:
                        pos_on_side()
                    for i in range(n):
                        tag = f"{kind}.{i}.mha"
                        P = self._act(tag + ".P", (posx.shape[0], d))
                        ops.linear_fwd(posx, self.W(tag + ".wpos"), P, compute=self.cmp)
                        self._P_ahead[tag] = P
                return run
            self._pos_ev = {}
            if c.pre_blocks > 0:       # the speech tokens' own table: the first T_mel rows of the encoder's
                self._pos_ev["pre"] = self._side(project("pre", pos_e[:Tm], c.pre_blocks), want_event="pos.pre")
            self._pos_ev["enc"] = self._side(project("enc", pos_e, c.enc_blocks), want_event="pos.enc")
            if c.has_decoder:
                self._pos_ev["dec"] = self._side(project("dec", pos_d, c.dec_blocks), want_event="pos.dec")     # (behind the decoder-side weight cast)
        if c.pre_blocks > 0:
            kms = ws.get("keymask.pre", (B, Tm), torch.uint8)
            kms.copy_(batch["speech_mask"].reshape(B, Tm).view(torch.uint8))
            self._fused_now, self._fused_train_now = self._attn_choice(B, Tm, need_grad)
            x = xsp
            for i in range(c.pre_blocks):
                x = self.block_fwd(f"pre.{i}", x, pos_e[:Tm], kms, B, Tm)
            self._fused_now, self._fused_train_now = main_path
            xs = ws.get("emb.xs", (B * T, d))
            ops.concat_rows(x, xst, xs, B, Tm, Tp, d)
        x = self._encode(xs, B, T, (pos_e, keymask), (pos_d, keymask), self._drop(pp, "dec.x"))
        return self._finish(x, speech2, masked, need_grad, gscale)

    def _finish(self, x, speech2, masked, need_grad, gscale):
        """Head and loss behind the last block's LayerNorm: what forward() returns."""
        c, ws = self.c, self.ws
        B, Tm, _, _ = self.dims
        hs, before, after = self._head(x)
        loss = ws.get("head.loss", (1,))
        scratch = ws.get("head.lscratch", (ops.loss_scratch_floats(B * Tm),))
        db = ws.get("head.dbefore", (B * Tm, c.odim)) if need_grad else None
        da = ws.get("head.dafter", (B * Tm, c.odim)) if (need_grad and after is not None) else None
        ops.mlm_loss(before, after, speech2, masked, loss, db, da, scratch, l2=c.lsm_weight > 50, gscale=gscale)
        self.sv["head"] = (hs, before, after, db, da)
        return dict(loss=loss, before=before.view(B, Tm, c.odim),
                    after=(after if after is not None else before).view(B, Tm, c.odim))

    def _encode(self, x, B, T, enc, dec, dec_drop=None, **ragged):
        """Encoder blocks and after_norm, then (unless no_decoder, sedit_model.py:356-362: the head reads the encoder's output as
        it is) the decoder (conformer/encoder.py:568-614): x * sqrt(d), its own rel-pos table.  enc / dec = (pos, keymask);
        ragged: lens / pos_rows of the encoder's blocks, lens of the decoder's."""
        c = self.c
        for i in range(c.enc_blocks):
            x = self.tblock_fwd(f"enc.{i}", x, enc[1], B, T) if self.transformer else self.block_fwd(f"enc.{i}", x, *enc, B, T, **ragged)
        x = self._ln_fwd("enc.after", x, "enc.after", out_dtype=torch.float32)
        if c.has_decoder:
            xd = self.ws.get("dec.in", (B * T, c.adim))
            if self.transformer:      # MLMDecoder.embed: PositionalEncoding over the joined row, t = 0 .. T - 1
                ops.scale_add_pos(x, self.pe_abs, xd, B, T, c.adim, math.sqrt(c.adim), drop=dec_drop or (0.0, 0))
            elif dec_drop:
                ops.dropout(x, xd, dec_drop[0], dec_drop[1], scale=math.sqrt(c.adim))
            else:
                ops.scale(x, xd, math.sqrt(c.adim))
            x = xd
            self._wait_cast("_cast_ev")       # decoder / head shadows cast on the side stream (refresh_weights)
            for i in range(c.dec_blocks):
                x = self.tblock_fwd(f"dec.{i}", x, dec[1], B, T) if self.transformer else \
                    self.block_fwd(f"dec.{i}", x, *dec, B, T, lens=ragged.get("lens"))
            x = self._ln_fwd("dec.after", x, "dec.after", out_dtype=torch.float32)
        return x

    def _forward_rows_alone(self, batch, need_grad, lens):
        """forward() of a padded batch whose row b comes out as the reference gives it for that row passed ALONE (its driver is
        B = 1 throughout): the pre-speech blocks run ragged at slens, then the rows are PACKED -- row b = its sl_b speech tokens
        with its tl_b text tokens directly behind them (a3t_concat_rows_ragged), as in the row alone, where no padding separates
        the two -- and every block runs ragged at n_b = sl_b + tl_b.  The encoder's positional rows are cat(pe[:sl_b], pe[:tl_b])
        per row (block_fwd(pos_rows=)), the decoder's pe[:n_b] are a prefix of the shared table; every block projects its own,
        on the main stream.  The speech and text masks are not read: the lengths say the same.  The first Tm rows of a packed
        row hold its speech frames for the head (_head(slens)).  Rows of before / after behind sl_b are unspecified (finite).
        No loss."""
        c, ws, (slens, tlens) = self.c, self.ws, lens
        if self.transformer:
            raise NotImplementedError("lens= (rows='alone'): ragged rows are implemented for the conformer blocks only, not for a "
                                      "transformer model")
        self._need_grad = bool(need_grad)
        self._check_ragged(slens, batch["speech"].shape[0])
        self._check_ragged(tlens, batch["speech"].shape[0])
        self._fused_now = self._fused_train_now = False
        speech2, text, masked = self._begin(batch, need_grad)
        (B, Tm, Tp, T), d = self.dims, c.adim
        _, x, xst = self._prologue(batch, speech2, text, masked, split=True)
        for i in range(c.pre_blocks):
            x = self.block_fwd(f"pre.{i}", x, self.pe[:Tm], None, B, Tm, lens=slens)
        xs = ws.get("emb.xs", (B * T, d))
        ops.concat_rows_ragged(x, xst, xs, slens, tlens, B, Tm, Tp, d)
        n = ws.get("emb.nlens", (B,), torch.int32)
        torch.add(slens, tlens, out=n)
        x = self._encode(xs, B, T, (self.pe[:max(Tm, Tp)], None), (self.pe[:T], None), lens=n, pos_rows=(slens, tlens, Tm, Tp))
        _, before, after = self._head(x, slens)
        return dict(loss=None, before=before.view(B, Tm, c.odim), after=(after if after is not None else before).view(B, Tm, c.odim))

    def backward(self, on_group_done=None):
        """Accumulates d loss / d param (times the gscale given to forward) into store.grad.
        on_group_done(first_param_name) is called each time every parameter at or above that flat
        offset has its final gradient (hook for overlapping the gradient all-reduce)."""
        hook = on_group_done or (lambda name: None)

        def done(name):          # every gradient at or above `name` is final once the side streams have drained: a hook that
            hook(name)           # consumes gradients calls join_side() first (no join at all without one -- it stalls the main stream)
        c, p, gr, ws = self.c, self.store.p, self.store.g, self.ws
        B, Tm, Tp, T = self.dims
        d = c.adim
        cmp = self.cmp
        self._wait_cast("_cast_ev")
        self._wait_cast("_wt_ev")         # transposed weight shadows cast on the side stream (refresh_weights)
        self._arena_clear("bwd64")
        self._arena_clear("bwd32")
        hs, before, after, db, da = self.sv["head"]
        pad = (c.postnet_filts - 1) // 2
        if c.postnet_layers > 0:
            g = da                                    # grad wrt last BN output (fp32)
            for l in reversed(range(c.postnet_layers)):
                W = self.W(f"post.{l}.w")
                oc = W.shape[0]
                last = (l == c.postnet_layers - 1)
                dz = ws.get(f"tmp.post.dz{oc}.{l}", (B * Tm, oc))      # (per layer: the side stream reads it after the main stream moved on)
                pdr = self._drop(c.postnet_dropout_rate, f"post.{l}")
                if pdr:
                    gd = ws.get(f"tmp.post.gd{oc}", (B * Tm, oc))
                    ops.dropout(g, gd, *pdr)
                    g = gd
                self._bn_bwd(f"post.{l}", g, f"post.{l}.bn", ACT_NONE if last else ACT_TANH, dz)
                if self.bf16:
                    dz16 = ws.get(f"tmp.post.dz16.{oc}.{l}", (B * Tm, oc), torch.bfloat16)
                    ops.cast_bf16(dz, dz16)
                    dz = dz16
                yin = self.sv[f"post.{l}"]
                ic = yin.shape[1]
                # (weight gradients of the head: the side stream is idle at the start of the backward)
                self._side(
                    lambda dz=dz, yin=yin, l=l: ops.conv_bwd_weight(dz, yin, gr[f"post.{l}.w"], Tm, pad, compute=cmp))
                gi = ws.get(f"tmp.post.g{l % 2}.{ic}", (B * Tm, ic))
                ops.conv_bwd_data(dz, W, gi, Tm, pad, compute=cmp)
                g = gi
            ops.axpy(da, db, 1.0)                     # after = before + postnet(before)
            ops.axpy(g, db, 1.0)
        dba = db
        if self.bf16:
            dba = ws.get("tmp.db16", (B * Tm, c.odim), torch.bfloat16)
            ops.cast_bf16(db, dba)
        dhs = ws.get("tmp.dhs", (B * Tm, d))
        ops.linear_bwd_data(dba, self.W("sfc.w"), dhs, compute=cmp)
        self._side(lambda: ops.linear_bwd_weight(dba, hs, gr["sfc.w"], compute=cmp))
        self._bias_grad(db, gr["sfc.b"])
        done("sfc.w")
        g = ws.get("grad.x", (B * T, d), zero=True)
        g16 = self._g16(g)
        ops.slice_rows(g, dhs, B, T, Tm, d, reverse_add=True)
        tr = self.transformer

        def closing(stack, n):      # a transformer stack ends in an FFN, not in a block LayerNorm: its bias gradient comes from after_norm's backward
            return ((gr[f"{stack}.{n - 1}.ff.b2"], 1.0), f"{stack}.{n - 1}.ff.o") if tr else (None, None)

        def stack_bwd(stack, n):
            for i in reversed(range(n)):
                if tr:
                    self.tblock_bwd(f"{stack}.{i}", g, B, T, f"{stack}.{i - 1}" if i > 0 else None)
                    done(f"{stack}.{i}.mha.ln.g")
                else:
                    self.block_bwd(f"{stack}.{i}", g, B, T)
                    done(f"{stack}.{i}.ffm.ln.g")
        if c.has_decoder:
            self._ln_bwd("dec.after", g, "dec.after", None, g, g16, *closing("dec", c.dec_blocks))
            stack_bwd("dec", c.dec_blocks)
            dd = self._drop(c.positional_dropout_rate, "dec.x")
            if dd:
                ops.dropout(g, g, dd[0], dd[1], scale=math.sqrt(d))
            else:
                ops.scale(g, g, math.sqrt(d))
        self._ln_bwd("enc.after", g, "enc.after", None, g, g16, *closing("enc", c.enc_blocks))
        stack_bwd("enc", c.enc_blocks)
        gs = gt = None
        if c.pre_blocks > 0:     # the gradient of the concatenation: the speech part goes back through the pre-speech blocks
            gs, gt = ws.get("grad.xsp", (B * Tm, d)), ws.get("grad.xst", (B * Tp, d))
            ops.split_rows(g, gs, gt, B, Tm, Tp, d)
            for i in reversed(range(c.pre_blocks)):
                self.block_bwd(f"pre.{i}", gs, B, Tm)
                done(f"pre.{i}.ffm.ln.g")
        # --- prologue backward
        if "spk" in self.sv:     # d Linear(spembs): per-utterance column sums of the gradient of the token stream
            se = self.sv["spk"]
            dspk = ws.get("tmp.dspk", (B, d), zero=True)
            if gs is None:
                ops.segment_colsum(g, dspk, B, T)
            else:                # (added to both parts at the prologue: speech-side + text-side sums)
                ops.segment_colsum(gs, dspk, B, Tm)
                if Tp > 0:
                    ops.segment_colsum(gt, dspk, B, Tp)
            ops.linear_bwd_weight(dspk, se, gr["spk.w"], compute=F32)
            self._bias_grad(dspk, gr["spk.b"])
        xm, e, text, spos, tpos, masked, speech2 = self.sv["embed"]
        de = ws.get("tmp.de", (B * Tm, d))
        dseg = gr["seg"] if c.segment_emb else None
        pdrop = c.positional_dropout_rate
        if tr:
            dal = self._alphas(gr)
            part = ws.get("tmp.dalpha", (ops.embed_finish_abs_partials(B, Tm, Tp, d),)) if dal is not None else None
            ops.embed_finish_abs_bwd(g, e, text, spos, tpos, self.pe_abs, de, gr["temb"], dseg, dal, part, B, Tm, Tp, d, c.vocab,
                                     c.seg_table, math.sqrt(d), drop=self._drop(pdrop, "emb.x") or (0.0, 0))
        elif gs is None:
            ops.embed_finish_bwd(g, e, text, spos, tpos, de, gr["temb"], dseg, B, Tm, Tp, d, c.vocab, c.seg_table,
                                 math.sqrt(d), drop=self._drop(pdrop, "emb.x") or (0.0, 0))
        else:
            ops.embed_finish_bwd(gs, e, text, spos, tpos, de, gr["temb"], dseg, B, Tm, 0, d, c.vocab, c.seg_table,
                                 math.sqrt(d), drop=self._drop(pdrop, "emb.x") or (0.0, 0))
            ops.embed_finish_bwd(gt, e, text, spos, tpos, de, gr["temb"], dseg, B, 0, Tp, d, c.vocab, c.seg_table,
                                 math.sqrt(d), drop=self._drop(pdrop, "emb.xt") or (0.0, 0))
        de0 = ws.get("tmp.de0", (B * Tm, d))
        de16 = ws.get("tmp.de016", (B * Tm, d), torch.bfloat16) if self.bf16 else None
        self._ln_bwd("emb.ln", de, "emb.ln", None, de0, de16, (gr["emb.b"], 1.0))
        dea = de16 if self.bf16 else de0
        ops.linear_bwd_weight(dea, xm, gr["emb.w"], compute=cmp)
        dxm = ws.get("tmp.dxm", (B * Tm, c.idim))
        ops.linear_bwd_data(dea, self.W("emb.w"), dxm, compute=cmp)
        s64 = self.scratch64[:c.idim]
        s64.zero_()
        ops.col_reduce(dxm, s64, rowmask=masked.view(-1), mode=0)
        ops.f64_to_f32_add(s64, gr["mask_feature"], 1.0)
        done(next(iter(self.store.offsets)))      # (the first entry of the layout: "seg", or "mask_feature" without a segment table)
        self.join_side()        # every gradient is final on the caller's stream when backward returns
