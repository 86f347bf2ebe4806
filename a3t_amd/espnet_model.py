"""ESPnet2 model-plugin surface of the A3T masked-mel model, backed by the HIP engine.

Mirror of ``ESPnetMLMEncAsDecoderModel`` / ``ESPnetMLMModel`` (espnet2/tts/sedit/sedit_model.py:
forward :155-187, _forward :350-375, inference :239-284, collect_feats :125-128): same call
signature, same ``(loss, stats, weight)`` return contract (AbsESPnetModel,
espnet2/train/abs_espnet_model.py:9-42), same ``state_dict`` keys/shapes, so
``Trainer.train_one_epoch`` (espnet2/train/trainer.py:545,610) can drive it unchanged:
``loss.backward()`` runs the hand-written backward schedule and leaves gradients in ``p.grad``
(in ``eval()`` mode too, when grad is enabled: sedit_inference.py's dynamic_evaluation relies on it).

There is no CPU execution path: calling forward without the HIP library / a GPU raises.
"""
from collections import OrderedDict
from typing import Dict, List, Tuple, Union

import torch

from .config import A3TConfig
from .conformer import COMPUTE_MODES
from .params import ParamStore


class _Namespace:
    pass


class _TrainStep(torch.autograd.Function):
    """One autograd node for the whole model: forward = engine.forward, backward = engine.backward.
    The node's inputs are all parameters, so autograd (and a DistributedDataParallel wrapper's
    reduction hooks, trainer.py:250-265) see an ordinary gradient per parameter."""

    @staticmethod
    def forward(ctx, model, batch, *params):
        out = model._engine().forward(batch, need_grad=True)
        ctx.model = model
        model._last = out
        return out["loss"].clone()

    @staticmethod
    def backward(ctx, gloss):
        from . import ops
        m = ctx.model
        st = m.store
        st.grad.zero_()
        m._engine().backward()
        ops.scale_dev(st.grad, st.grad, gloss.reshape(-1)[:1].contiguous().float())   # d(total)/d(loss), no host sync
        return (None, None) + tuple(st.g[n] for n in m._params)


class ESPnetMLMEncAsDecoderModel(torch.nn.Module):
    def __init__(self, token_list: Union[Tuple[str, ...], List[str]], odim: int, feats_extract, normalize,
                 config: A3TConfig, device="cpu", compute: str = "f32", **model_conf):
        super().__init__()
        self.token_list = list(token_list)
        self.odim = odim
        self.feats_extract = feats_extract
        self.normalize = normalize            # stored, never applied (sedit_model.py:79)
        self.cfg = config
        if compute not in COMPUTE_MODES:      # (a typo must not reach the engine, nor the checks on self.compute, as another mode)
            raise ValueError(f"compute={compute!r}: expected one of {', '.join(map(repr, COMPUTE_MODES))}")
        self.compute = compute
        # torch.nn.Dropout semantics: the recipe's dropout sites are active in train() mode, off in eval() mode
        # (dropout=False builds a deterministic training engine: parity tests, finite-difference checks)
        self.dropout = bool(model_conf.get("dropout", True))
        self.mlm_prob = model_conf.get("mlm_prob", config.mlm_prob)
        self.mean_phn_span = model_conf.get("mean_phn_span", config.mean_phn_span)
        self.masking_schema = model_conf.get("masking_schema", "phn_span")
        self.ignore_id = -1
        self.encoder = _Namespace()           # attributes read by callers
        self.encoder._output_size = config.adim
        self.encoder.segment_emb = True if config.segment_emb else None      # (input_layer 'mlm': conformer/encoder.py:387)
        self.encoder.pre_speech_layer = config.pre_blocks
        self.decoder = _Namespace() if config.has_decoder else None           # (no_decoder: tasks/mlm.py:412-413)
        self._eng = {}
        self._last = None
        self._build_store(device)

    # ------------------------------------------------------------------ parameters
    def _build_store(self, device, state=None):
        self.store = ParamStore(self.cfg, device)
        if state is not None:
            self.store.load_state_dict(state)
        self._params = OrderedDict()
        for old in [k for k in self._parameters]:
            del self._parameters[old]
        for name, view in self.store.p.items():
            p = torch.nn.Parameter(view, requires_grad=True)
            self._params[name] = p
            self.register_parameter(name.replace(".", "__"), p)
        self._eng = {}

    def _apply(self, fn, *a, **k):
        """model.to(device) / .cuda(): migrate the flat store instead of per-tensor copies."""
        probe = fn(torch.zeros(1, device=self.store.device))
        if probe.device != self.store.device:
            self._build_store(probe.device, self.store.state_dict())
        if probe.dtype != torch.float32:
            raise NotImplementedError("master weights are fp32; pick bf16 compute with compute='bf16'")
        return self

    def _engine(self):
        from .engine import MLMEngine
        key = self.training
        if key not in self._eng:
            self._eng[key] = MLMEngine(self.cfg, self.store, compute=self.compute, training=self.training,
                                       dropout=self.dropout and self.training)
            if (not key) in self._eng:       # share activation buffers between train / eval schedules
                self._eng[key].ws = self._eng[not key].ws
        return self._eng[key]

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        sd = self.store.state_dict()
        out = destination if destination is not None else OrderedDict()
        for k, v in sd.items():
            out[prefix + k] = v
        return out

    def load_state_dict(self, state_dict, strict: bool = True):
        missing, unexpected = self.store.load_state_dict(state_dict, strict=strict)
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    # ------------------------------------------------------------------ plugin surface
    def collect_feats(self, speech, speech_lengths, text, text_lengths, masked_position, speech_mask, text_mask,
                      speech_segment_pos, text_segment_pos, y_masks=None) -> Dict[str, torch.Tensor]:
        return {"feats": speech, "feats_lengths": speech_lengths}

    def _batch(self, speech, text, masked_position, speech_mask, text_mask, speech_segment_pos, text_segment_pos,
               spembs=None):
        dev = self.store.device
        b = dict(speech=speech.to(dev, torch.float32), text=text.to(dev), masked_position=masked_position.to(dev),
                 speech_mask=speech_mask.to(dev), text_mask=text_mask.to(dev),
                 speech_segment_pos=speech_segment_pos.to(dev), text_segment_pos=text_segment_pos.to(dev))
        if spembs is not None and self.cfg.spk_embed_dim > 0:
            b["spembs"] = spembs.to(dev, torch.float32)
        if self.compute == "bf16":
            b = self._pad_to_dma_granule(b)
        return b

    @staticmethod
    def _pad_to_dma_granule(b):
        """The bf16 kernels move 16-byte granules, so T_mel and T_mel + T_phn must be multiples of 8.  Real batches are
        padded to the longest utterance anyway (collate_fn.py:197-214); here the padding is simply extended: extra speech
        frames are 0 with speech_mask / masked_position False and segment id 0, extra phones are the pad id 0 with
        text_mask False -- exactly what the reference's collate produces for a batch whose longest utterance is a few
        frames longer.  (As in the reference, padded positions still enter the BatchNorm statistics.)"""
        Tm, Tp = b["speech"].shape[1], b["text"].shape[1]
        pm = (-Tm) % 8
        pp = (-(Tm + pm + Tp)) % 8
        if pm == 0 and pp == 0:
            return b
        F = torch.nn.functional
        out = dict(b)
        if pm:
            out["speech"] = F.pad(b["speech"], (0, 0, 0, pm))
            out["masked_position"] = F.pad(b["masked_position"], (0, pm), value=False)
            out["speech_mask"] = F.pad(b["speech_mask"], (0, pm), value=False)
            out["speech_segment_pos"] = F.pad(b["speech_segment_pos"], (0, pm), value=0)
        if pp:
            out["text"] = F.pad(b["text"], (0, pp), value=0)
            out["text_mask"] = F.pad(b["text_mask"], (0, pp), value=False)
            out["text_segment_pos"] = F.pad(b["text_segment_pos"], (0, pp), value=0)
        return out

    def forward(self, speech, text, masked_position, speech_mask, text_mask, speech_segment_pos, text_segment_pos,
                y_masks=None, speech_lengths=None, text_lengths=None, spembs=None):
        """spembs (B, spk_embed_dim): speaker x-vectors; used only by a model built with spk_embed_dim > 0 (an extension:
        the reference model ignores them, sedit_model.py:246)."""
        batch_size = speech.shape[0]
        batch = self._batch(speech, text, masked_position, speech_mask, text_mask, speech_segment_pos,
                            text_segment_pos, spembs)
        if torch.is_grad_enabled():
            # train() and eval() alike, as in the reference model (its dynamic evaluation calls eval() and then
            # loss.backward()): the eval engine runs without dropout and with BatchNorm on its running statistics.  Under
            # torch.no_grad() -- and in inference() -- the pass is forward-only: no saved tensors, no transposed weight shadows.
            loss = _TrainStep.apply(self, batch, *self._params.values())
        else:
            loss = self._engine().forward(batch, need_grad=False)["loss"].clone()
            self._last = None
        stats = dict(loss=loss.detach(), loss_mlm=loss.detach(), loss_copy=None)
        weight = torch.tensor([batch_size], dtype=torch.long, device=loss.device)
        return loss.reshape(1), {k: (v.reshape(1) if v is not None else None) for k, v in stats.items()}, weight

    def inference(self, speech, text, masked_position, speech_mask, text_mask, speech_segment_pos, text_segment_pos,
                  span_boundary, y_masks=None, speech_lengths=None, text_lengths=None, feats=None, spembs=None,
                  sids=None, lids=None, threshold=0.5, minlenratio=0.0, maxlenratio=10.0,
                  use_teacher_forcing: bool = False) -> Dict[str, torch.Tensor]:
        """Teacher-forcing branch only (the reference's step-by-step branch is dead code,
        sedit_model.py:285-317): one forward, splice the predicted span into the input mels."""
        if not use_teacher_forcing:
            raise NotImplementedError("only use_teacher_forcing=True is functional in the reference")
        batch = self._batch(speech, text, masked_position, speech_mask, text_mask, speech_segment_pos,
                            text_segment_pos, spembs)
        out = self._engine().forward(batch, need_grad=False)
        zs = out["after"]
        s, e = int(span_boundary[0]), int(span_boundary[1])
        sp = batch["speech"][:, :speech.shape[1]]          # (bf16 mode may have extended the padding)
        return dict(feat_gen=[sp[:, :s], zs[0][s:e].clone(), sp[:, e:]])

    def inference_batch(self, speech, text, masked_position, speech_mask, text_mask, speech_segment_pos, text_segment_pos,
                        span_boundary, spembs=None, use_teacher_forcing: bool = True, rows: str = "batch",
                        max_score_elems: int = 1 << 24, span_counts=None):
        """Teacher-forced infill of a whole batch: one forward-only pass, then a3t_splice_spans writes, per row b,
        out[b][t] = after[b][t] for span_boundary[b][0] <= t < span_boundary[b][1], speech[b][t] for the other valid frames
        and 0 behind the row's length speech_mask[b].sum() (the batch's speech_lengths are raw samples, as in the reference).
        Returns (out (B, Tmax, odim) fp32, lengths (B,) int32), both on the device.

        span_boundary: (B, 2), one span per row, as above; or several spans per row -- a list of per-row lists of [s, e]
        (a row may have none), or a (B, S, 2) tensor with span_counts (B,), how many of a row's S entries count.  Frame t of
        row b then takes after[b][t] iff it lies in any of the row's spans (a3t_splice_spans_multi); rows="alone" carries
        the lists through its chunks.

        rows="batch" (the default): a row is what the reference's collate function and model give for that row IN that batch.
        That is not the same request run alone, in the reference either: the convolution module and the FFN convolutions do not
        mask padded frames, padding separates a short row's speech and text tokens, and the legacy rel_shift and the encoder's
        positional table depend on the padded lengths.  The model is trained on exactly such batches.

        rows="alone": row b is computed as the reference's B = 1 driver computes it, from the row's own speech_mask / text_mask
        lengths (prefix masks; MLMEngine._forward_rows_alone), to fp32 rounding -- not bit for bit.  fp32 or bf16x3 compute (fp32
        storage both), eval mode.
        The rows are sorted by tokens n_b and cut into chunks with B * heads * n_max^2 <= max_score_elems (each of the three
        score-sized tensors of the materialised attention); a chunk of one row takes the plain B = 1 pass at the row's exact
        lengths.  The device lengths come from the masks without a host synchronisation; the chunking needs them on the host,
        which is free when the masks arrive as host tensors and is skipped when the padded batch fits the cap as it is."""
        if not use_teacher_forcing:
            raise NotImplementedError("only use_teacher_forcing=True is functional in the reference")
        if rows not in ("batch", "alone"):
            raise ValueError(f"rows must be 'batch' or 'alone', got {rows!r}")
        B, Tmax = speech.shape[0], speech.shape[1]
        sb, nsp = self._span_arguments(span_boundary, span_counts, B)
        if rows == "alone":
            if self.cfg.block == "transformer":
                raise NotImplementedError("rows='alone' (lens= on the engine): ragged rows are implemented for the conformer blocks "
                                          "only, not for a transformer model")
            if self.compute not in ("f32", "bf16x3") or self.training:
                raise ValueError("rows='alone' needs a model built with compute='f32' or 'bf16x3' in eval mode "
                                 f"(compute={self.compute!r}, training={self.training}): the fused bf16 attention forward has "
                                 "no per-row rel_shift")
            host = None
            if not speech_mask.is_cuda and not text_mask.is_cuda:
                host = (speech_mask.reshape(B, -1).sum(-1).tolist(), text_mask.reshape(B, -1).sum(-1).tolist())
        batch = self._batch(speech, text, masked_position, speech_mask, text_mask, speech_segment_pos, text_segment_pos, spembs)
        dev = self.store.device
        spans = sb.to(torch.int32).contiguous().to(dev, non_blocking=True)
        if nsp is not None:
            nsp = nsp.to(torch.int32).contiguous().to(dev, non_blocking=True)
        if rows == "alone":
            return self._infill_rows_alone(batch, spans, host, int(max_score_elems), nsp)
        out = self._engine().forward(batch, need_grad=False)
        sp = batch["speech"].contiguous()                     # (bf16 mode may have extended the padding)
        res = torch.empty(B, Tmax, sp.shape[2], dtype=torch.float32, device=dev)
        lens = torch.empty(B, dtype=torch.int32, device=dev)
        self._splice(out["after"].contiguous(), sp, batch["speech_mask"].contiguous().view(B, -1), spans, nsp, res, lens)
        return res, lens

    @staticmethod
    def _span_arguments(span_boundary, span_counts, B):
        """inference_batch's span_boundary -> (spans, counts): ((B, 2), None) for one span per row, ((B, S, 2), (B,)) for span
        lists.  A list whose rows are lists of [s, e] pairs (or empty) is a list of span lists."""
        if torch.is_tensor(span_boundary):
            sb = span_boundary
            if sb.dim() == 3:
                if sb.shape[0] != B or sb.shape[1] < 1 or sb.shape[2] != 2 or span_counts is None:
                    raise ValueError(f"span_boundary (B, S, 2) = ({B}, S >= 1, 2) comes with span_counts (B,), got "
                                     f"{tuple(sb.shape)} and span_counts={span_counts!r}")
                nsp = span_counts if torch.is_tensor(span_counts) else torch.tensor([int(n) for n in span_counts])
                if nsp.numel() != B:
                    raise ValueError(f"span_counts must be (B,) = ({B},), got {tuple(nsp.shape)}")
                return sb, nsp.reshape(B)
        else:
            rows_ = list(span_boundary)
            if any(len(r) == 0 or not isinstance(r[0], (int, float)) and hasattr(r[0], "__len__") for r in rows_):
                if len(rows_) != B:
                    raise ValueError(f"span_boundary: {len(rows_)} span lists for {B} rows")
                S = max(1, max(len(r) for r in rows_))
                sb = torch.zeros(B, S, 2, dtype=torch.int32)
                for b, r in enumerate(rows_):
                    for k, (s, e) in enumerate(r):
                        sb[b, k, 0], sb[b, k, 1] = int(s), int(e)
                return sb, torch.tensor([len(r) for r in rows_], dtype=torch.int32)
            sb = torch.tensor([[int(s), int(e)] for s, e in rows_])
        if span_counts is not None:
            raise ValueError("span_counts belongs to a (B, S, 2) span_boundary")
        if sb.shape != (B, 2):
            raise ValueError(f"span_boundary must be (B, 2) = ({B}, 2), got {tuple(sb.shape)}")
        return sb, None

    @staticmethod
    def _splice(after, speech, mask, spans, nsp, out, lens):
        from . import ops
        if nsp is None:
            ops.splice_spans(after, speech, mask, spans, out, lens)
        else:
            ops.splice_spans_multi(after, speech, mask, spans, nsp, out, lens)

    _ROW_KEYS = ("speech", "masked_position", "speech_mask", "speech_segment_pos")      # [B][T_mel]..., the rest [B][T_phn]...

    def _infill_rows_alone(self, batch, spans, host, max_score_elems, nsp=None):
        """inference_batch(rows="alone") behind the argument checks.  host: (frames, phones) per row as host lists, or None;
        nsp: the rows' span counts when spans is (B, S, 2), None for (B, 2)."""
        from .conformer import score_chunks
        dev, eng = self.store.device, self._engine()
        speech = batch["speech"]
        B, Tm, odim = speech.shape
        Tp = batch["text"].shape[1]
        b = dict(batch, speech_mask=batch["speech_mask"].reshape(B, Tm), text_mask=batch["text_mask"].reshape(B, Tp))
        slens = b["speech_mask"].sum(-1, dtype=torch.int32)
        tlens = b["text_mask"].sum(-1, dtype=torch.int32)
        res = torch.empty(B, Tm, odim, dtype=torch.float32, device=dev)
        lens = torch.empty(B, dtype=torch.int32, device=dev)

        def run(sub, sp, lp, out_rows, out_lens, cnt=nsp):
            out = eng.forward(sub, need_grad=False, lens=lp)
            self._splice(out["after"].contiguous(), sub["speech"].contiguous(), sub["speech_mask"].contiguous(), sp, cnt,
                         out_rows, out_lens)

        if B > 1 and host is None and B * self.cfg.heads * (Tm + Tp) ** 2 <= max_score_elems:
            # one chunk as the batch stands: nobody needs the lengths on the host
            run(b, spans, (slens, tlens), res, lens)
            return res, lens
        if host is None:
            both = torch.stack([slens, tlens]).tolist()      # the one host synchronisation: the chunking needs the lengths
            host = (both[0], both[1])
        sl, tl = [int(x) for x in host[0]], [int(x) for x in host[1]]
        for ch in score_chunks([s + t for s, t in zip(sl, tl)], self.cfg.heads, max_score_elems):
            tm, tp = max(sl[i] for i in ch), max(tl[i] for i in ch)
            idx = torch.tensor(ch, dtype=torch.long).to(dev, non_blocking=True)
            sub = {}
            for k, v in b.items():      # the chunk's rows, cut to the chunk's longest on both sides
                v = v.index_select(0, idx)
                sub[k] = v if k == "spembs" else v[:, :(tm if k in self._ROW_KEYS else tp)].contiguous()
            r = torch.empty(len(ch), Tm, odim, dtype=torch.float32, device=dev)
            ln = torch.empty(len(ch), dtype=torch.int32, device=dev)
            # a chunk of one row: the plain B = 1 pass at the row's exact lengths
            lp = None if len(ch) == 1 else (slens.index_select(0, idx), tlens.index_select(0, idx))
            run(sub, spans.index_select(0, idx).contiguous(), lp, r, ln, None if nsp is None else nsp.index_select(0, idx))
            res.index_copy_(0, idx, r)
            lens.index_copy_(0, idx, ln)
        return res, lens
