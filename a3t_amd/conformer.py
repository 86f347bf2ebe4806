"""A stack of Conformer blocks on liba3t_hip: feed-forward, legacy rel-pos self-attention and convolution module, forward and
hand-derived backward, with what a block needs around it -- positional table, bf16 weight shadows, GEMM plans, LayerNorm /
BatchNorm helpers, dropout keys -- and EngineOptions, the one record of the A3T_* switches.  ConformerStack launches kernels in
the order StepSchedule allows; it must not know what model the blocks sit in (no prologue, head or loss: engine.py, and the
FastSpeech2 models of duration.py / fs2_tts.py, which run their blocks on a bare stack).
A stack built from a config with block = "transformer" runs the transformer EncoderLayer instead (tblock_fwd / tblock_bwd: plain
MultiHeadedAttention, one position-wise FFN with residual scale 1.0, no LayerNorm behind the block).

Three numeric modes:
  compute="f32"  : everything fp32, GEMMs on the exact-fp32 MFMA  (parity path, 1e-4)
  compute="bf16x3" : the fp32 path -- same storage, same schedule, same fp32-only kernels -- with every GEMM that follows the
                   mode on three bf16 MFMA products per fp32 product (A3T_BF16X3: operands split into bf16 hi + lo in the
                   loader, operands carried to 2^-16 where bf16 has 2^-8)
  compute="bf16" : tensors that feed GEMMs are stored in bf16 (LayerNorm outputs, FFN hidden, q/k/v,
                   attention probabilities, ...), weights are cast to a bf16 shadow once per step,
                   GEMMs run on the bf16 MFMA with fp32 accumulation; the residual stream, all
                   normalisation statistics, softmax, loss, gradients of parameters and the
                   optimizer stay fp32  (throughput path, 1e-2)
"""
import math
import os
import zlib
from dataclasses import dataclass

import torch

from . import ops
from ._lib import ACC_ADD, ACC_ATOMIC, ACC_STORE, ACT_RELU, ACT_SWISH, BF16, BF16X3, F32
from .config import A3TConfig
from .params import ParamStore
from .schedule import StepSchedule


def legacy_pe_table(c: A3TConfig) -> torch.Tensor:
    """LegacyRelPositionalEncoding table (transformer/embedding.py:59-80 with reverse=True): a
    constant computed once on the host with the same fp32 formula, row t = PE(max_len-1-t)."""
    d = c.adim
    position = torch.arange(c.max_len - 1, -1, -1.0, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe = torch.zeros(c.max_len, d)
    pe[:, 0::2] = torch.sin(position * div)
    pe[:, 1::2] = torch.cos(position * div)
    return pe


def score_chunks(lengths, heads, max_score_elems):
    """Indices of `lengths` sorted by length and cut into consecutive chunks with B * heads * Tmax^2 <= max_score_elems (Tmax =
    the chunk's longest = last row), the size of a score tensor of the materialised attention; a row too long for the cap runs
    alone."""
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    out, cur = [], []
    for i in order:
        if cur and (len(cur) + 1) * heads * lengths[i] ** 2 > max_score_elems:
            out.append(cur)
            cur = []
        cur.append(i)
    if cur:
        out.append(cur)
    return out


@dataclass
class EngineOptions:
    """The engine's switches, one field per A3T_* variable (table in INTEGRATION.md).  The environment is read once, here,
    when a stack is built without options; the stack reads this record at every call, so a field may be flipped on a live
    engine (the ring depth and the streams aside, which exist from the constructor on).  Every "off" is the A/B twin."""
    side_stream: bool = True        # weight gradients (and other work that feeds nothing soon) on a second HIP stream
    side2: bool = True              # a stream of its own for what the main stream joins inside the sub-layer (dV, dK)
    side_depth: int = 48            # scratch sets the main stream may run ahead by (at least 2)
    wgrad_group: bool = True        # a block's Linear weight gradients in ONE launch (_lin_wgrad); needs a ring >= 8 deep
    # bf16 mode: the first postnet conv reads `before` (log-mel scale, |x| ~ 4: one bf16 ulp = 0.03) whose rounding the
    # five BatchNorm'ed postnet layers amplify.  Its forward therefore runs on (hi, lo) = (bf16(x), bf16(x - hi)): two
    # K = 5*80 bf16 GEMMs carry `before` to ~2^-17 (max error of `after` 6.2e-2 -> 4.3e-2 of scale); gradients use hi only.
    post_f32_first: bool = True
    # dS / dBD straight from the saved probabilities in one launch (a3t_attn_bwd_ds, which forms delta itself) instead of the
    # dprobs GEMM + softmax backward: dprobs is never stored.  configs[3] (d_k = 128): 61.25 ms per step against 62.33 / 62.30
    # with the materialised pair (profiles/r06_c4_ab.txt).
    attn_bwd_ds: bool = True
    # With attention dropout the fused training forward saves ONE score-sized tensor: exp(s - m_ref) with the dropout mask in its
    # sign bits (a3t_attn_fwd_train without probs_drop); a3t_attn_bwd_ds reads the mask there and the dV product clamps the
    # tagged elements to zero in its fragment registers (a3t_gemm_desc::a_signmask).  The dropped copy -- 161 MB written by
    # the forward per layer at configs[1], 415 MB at configs[3] -- is gone.  Off: two tensors.
    attn_signed: bool = True
    attn_dq_dual: bool = True       # dq = ds K + dbd P as one launch of the streaming kernel (_mha_bwd)
    attn_dbd_view: bool = True      # the compact dBD matrix is a strided view of dS, not a tensor (_mha_bwd)
    attn_dk_main: bool = True       # dK on the main queue behind dq where both run on the streaming kernel (_mha_bwd)
    # Fused legacy rel-pos attention forward (csrc/attn_fused.hip: scores, shifted position term, softmax, dropout and PV in one
    # launch, no logits in HBM), "auto" | "fwd" | "0".  Forward-only passes (need_grad=False) use a3t_attn_fwd when it launches
    # >= 64 workgroups (fwd: always; below that its latency floor loses to the materialised forward).  Training steps under "auto"
    # use a3t_attn_fwd_train, which also stores the un-normalised probabilities exp(s - m_ref), their dropped copy and 1 / row sum
    # for the backward (fused_attn_train = 0 switches that off, 2 lifts the 64-workgroup threshold so that the small-batch
    # parity fixtures go through it); the backward reads them (a3t_attn_bwd_ds or the materialised pair above).
    fused_attn: str = "auto"
    fused_attn_train: int = 1
    ffn_8p: bool = True             # FFN GEMMs on the persistent 8-phase / panel kernels where the library takes them (_ffn_plan)
    ffn_keep4: bool = True          # ... with the row-major keep image as the ReLU' mask of the panel kernel (_ffn_plan)
    lin_dgrad_t: bool = True        # Linear data gradients on the transposed weight shadow and the panel kernel (_lin_dgrad)
    fuse_ln_dropout: bool = True    # LayerNorm backward emits the next sub-layer's masked gradient (bf16, d % 128 == 0); no variable

    @classmethod
    def from_env(cls, environ=os.environ):
        fa, ft = environ.get("A3T_FUSED_ATTN", "auto"), environ.get("A3T_FUSED_ATTN_TRAIN", "1")
        if fa not in ("auto", "fwd", "0"):
            raise ValueError(f"A3T_FUSED_ATTN={fa!r}: expected auto, fwd or 0 (the flash backward behind '1' left the library in "
                             "round 5, tools/experiments/attn_flash_backward.patch)")
        on = {f: environ.get("A3T_" + f.upper(), "1") != "0" for f in
              ("side_stream", "side2", "wgrad_group", "post_f32_first", "attn_bwd_ds", "attn_signed", "attn_dq_dual",
               "attn_dbd_view", "attn_dk_main", "ffn_8p", "ffn_keep4", "lin_dgrad_t")}
        return cls(side_depth=max(2, int(environ.get("A3T_SIDE_DEPTH", "48"))), fused_attn=fa,
                   fused_attn_train=0 if ft == "0" else 2 if ft == "2" else 1, **on)


COMPUTE_MODES = {"f32": F32, "bf16": BF16, "bf16x3": BF16X3}     # compute= of a stack / engine / model -> a3t_gemm_desc.compute


class ConformerStack(StepSchedule):
    def __init__(self, cfg: A3TConfig, store: ParamStore, compute: str = "f32", training: bool = True,
                 dropout: bool = False, options: EngineOptions = None):
        """dropout=True enables the recipe's Dropout sites (dropout_rate / positional / attention rates of
        the config, 0.5 in the postnet) in training mode; masks come from a counter RNG keyed by
        (step seed, site), regenerated in the backward pass.  options=None: EngineOptions.from_env()."""
        self.opt = opt = options if options is not None else EngineOptions.from_env()
        super().__init__(store.device, opt.side_stream, opt.side2, opt.side_depth)
        self.c = cfg
        self.dropping = bool(dropout and training)
        self.step_seed = 0
        self.store = store
        if compute not in COMPUTE_MODES:
            raise ValueError(f"compute={compute!r}: expected one of {', '.join(map(repr, COMPUTE_MODES))}")
        self.compute = compute
        self.bf16 = (compute == "bf16")      # (False for "bf16x3": fp32 storage and the fp32 schedule)
        self.adt = torch.bfloat16 if self.bf16 else torch.float32   # storage of GEMM-operand activations
        self.cmp = COMPUTE_MODES[compute]
        self.training = training
        self.pe = legacy_pe_table(cfg).to(self.dev)
        # a transformer model's blocks (tblock_fwd / tblock_bwd): FFN residual scale 1.0 where the macaron pair has 0.5 each, and
        # absolute positions -- PositionalEncoding.pe is the same table in forward order (row t = PE(t); the legacy rel-pos class
        # inherits extend_pe and only reverses it)
        self.transformer = cfg.block == "transformer"
        self._ffs = 1.0 if self.transformer else 0.5
        self.pe_abs = self.pe.flip(0).contiguous() if self.transformer else None
        self.sv = {}
        self.scratch64 = torch.zeros(4 * max(cfg.ff, 3 * cfg.adim, cfg.postnet_chans, 64), dtype=torch.float64,
                                     device=self.dev)
        self.bn_momentum = 0.1
        # Linear weight gradients collected for one grouped launch (_lin_wgrad): 4 = one Conformer block's; needs the deep scratch ring
        self._wg_group = (2 if self.transformer else 4) if (self.bf16 and self.side is not None and self._depth >= 8 and opt.wgrad_group) else 1
        self._wg_pending, self._wg_slots = [], set()
        self._gm_ready = None
        self.colsum_slots = 16          # spread of the attention bias-gradient atomics (1 and 64 measured: slower / equal)
        self.fused_attn_fwd_only = self.bf16 and opt.fused_attn == "fwd"
        self.fused_attn_auto = self.bf16 and opt.fused_attn == "auto"
        self.fused_attn_train = self.bf16 and opt.fused_attn == "auto" and opt.fused_attn_train != 0
        self.fused_attn_train_min = 1 if opt.fused_attn_train == 2 else 64
        self._fused_now = self._fused_train_now = False
        # which attention forward each block of the last forward pass took ("fwd" = a3t_attn_fwd, "train" = a3t_attn_fwd_train,
        # "mat" = the materialised one), and the (B, T) it ran at
        self.attn_path, self.block_dims = {}, {}
        self._need_grad = training
        self._mode_tag = None
        if self.bf16:
            for n, v in (("adim", cfg.adim), ("ff", cfg.ff), ("idim", cfg.idim), ("odim", cfg.odim),
                         ("dk", cfg.dk), ("postnet_chans", cfg.postnet_chans or 8)):
                if v % 8:
                    raise ValueError(f"compute='bf16' needs {n} % 8 == 0 (16-byte DMA granules), got {v}")
            self.flat16 = torch.zeros(store.total, dtype=torch.bfloat16, device=self.dev)
            self.p16 = {k: self.flat16[o:o + math.prod(s)].view(s) for k, (o, s) in store.offsets.items()}
        self._ffn_plans = {}
        self._lin_plans = {}
        self._wt = {}        # transposed FFN weight shadows (8-phase data gradients), built on demand
        self._P_ahead, self._pos_ev = {}, None     # positional projections a model made ahead of its blocks (_mha_fwd)
        self._cast_ev = self._wt_ev = None
        dec = [o for k, (o, _) in store.offsets.items() if k.startswith("dec.")]
        self._cast_split = min(dec) if dec else 0        # flat offset of the first decoder parameter (a multiple of 64 elements)

    # ------------------------------------------------------------------ helpers
    def _drop(self, p, tag):
        """(p, key) of one dropout site for the current step, or None when dropout is off."""
        if not self.dropping or p <= 0.0:
            return None
        h = (zlib.crc32(tag.encode()) ^ ((self.step_seed * 0x9E3779B1) & 0xFFFFFFFF)) & 0xFFFFFFFF
        h = ((h ^ (h >> 16)) * 0x85EBCA6B) & 0xFFFFFFFF
        h = ((h ^ (h >> 13)) * 0xC2B2AE35) & 0xFFFFFFFF
        return (float(p), (h ^ (h >> 16)) & 0xFFFFFFFF)

    def _gm(self, g, tag, p, bias_grad, bias_scale):
        """Gradient entering a "residual + a*dropout(branch)" sub-layer: the GEMM operand (bf16 on the
        bf16 path) and, with dropout on, the masked gradient + the branch's output-bias gradient."""
        dr = self._drop(p, tag)
        if dr is None:
            return (self._g16(g) if self.bf16 else g)
        gm = self.ws.get(self._t("tmp.gm"), tuple(g.shape), self.adt)
        if self._gm_ready == tag:       # already produced by the LayerNorm backward that wrote g (fused epilogue)
            self._gm_ready = None
            return gm
        ops.dropout_bwd_cast(g, gm, dr[0], dr[1], colsum=bias_grad, colsum_scale=bias_scale)
        return gm

    def W(self, name):
        """GEMM-operand view of a parameter (bf16 shadow in bf16 mode)."""
        return self.p16[name] if self.bf16 else self.store.p[name]

    def refresh_weights(self):
        """bf16 shadows of the fp32 master weights, once per forward.  The flat buffer is laid out in forward order (prologue,
        encoder, decoder, head): only the part in front of the decoder is cast on the main stream; the rest, and the transposed
        shadows that only the backward reads, are cast on the (idle) side stream under the encoder's GEMMs -- the model's forward
        waits for the first before the decoder, its backward for the second (everything up front is 0.33 ms of HBM-bound
        kernels with nothing beside them: the one-stream schedule)."""
        self._cast_ev = self._wt_ev = None
        if not self.bf16:
            return
        split = self._cast_split if self.side is not None else 0
        flat, flat16 = self.store.flat, self.flat16
        wt = list(self._wt.values()) if self._need_grad else []      # transposed shadows feed data gradients only

        def transposed():
            for src_off, dst_off, _, tflat, shp in wt:
                ops.cast_bf16_conv_t(flat, tflat, src_off, dst_off, *shp)
        if split <= 0:
            ops.cast_bf16(flat, flat16)
            transposed()
            return
        ops.cast_bf16(flat[:split], flat16[:split])
        self._cast_ev = self._side(lambda: ops.cast_bf16(flat[split:], flat16[split:]), want_event="cast")
        if wt:
            self._wt_ev = self._side(transposed, want_event="wt")

    def _wait_cast(self, which):
        ev = getattr(self, which, None)
        if ev is not None:
            ev.wait_on(torch.cuda.current_stream())
            setattr(self, which, None)

    def _setup_wt(self, suf, shape):
        """Transposed, tap-reversed bf16 shadows of every weight `*.suf` of `shape` = [n][k][c] -> [c][k'][n] (Linear: k = 1, stored
        [n][c]): the data gradient of that conv / linear becomes a k-contiguous conv of the output gradient
        (a3t_cast_bf16_conv_t), which the 8-phase and the 384-column panel GEMMs can run.  One transposing cast per step for all
        of them; only built when one of those kernels would take the GEMM."""
        stored = (tuple(shape), (shape[0], shape[2])) if shape[1] == 1 else (tuple(shape),)
        names = [k for k in self.store.offsets if k.endswith("." + suf) and tuple(self.store.offsets[k][1]) in stored]
        if not names:
            return
        n = math.prod(shape)
        flat = torch.zeros(n * len(names), dtype=torch.bfloat16, device=self.dev)
        src = torch.tensor([self.store.offsets[k][0] for k in names], dtype=torch.int64, device=self.dev)
        dst = torch.arange(len(names), dtype=torch.int64, device=self.dev) * n
        views = {k: flat[i * n:(i + 1) * n].view(shape[2], shape[1], shape[0]) for i, k in enumerate(names)}
        self._wt[suf] = (src, dst, views, flat, tuple(shape))
        ops.cast_bf16_conv_t(self.store.flat, flat, src, dst, *shape)

    def _ffn_plan(self, M):
        """Which FFN GEMMs of an M-token batch go to the persistent 8-phase / panel kernels (the library's cost models decide,
        a3t_gemm_8p_supported / a3t_gemm_pn_supported): (keep, dgrad1, dgrad2, keep4).  keep = the keep-bit protocol (forward conv 1
        writes one bit per hidden activation, the data gradient of conv 2 reads it through the transposed w_2); dgrad1 / dgrad2 =
        the data gradient of conv 1 / conv 2 through the transposed w_1 / w_2; keep4 = dgrad2 masked by the row-major keep image.
        opt.ffn_8p off: none of them."""
        # keyed by what the probes depend on: the kernels' modes may change at run time (a3t_gemm_8p_mode / _pn_mode), and a
        # forward-only pass needs neither keep bits nor transposed weight shadows
        key = (M, self._need_grad, self._mode_tag, self.opt.ffn_8p, self.opt.ffn_keep4)
        if key not in self._ffn_plans:
            c = self.c
            keep = d1 = d2 = keep4 = False
            if self._need_grad and self.bf16 and self.dev.type == "cuda" and self.opt.ffn_8p:
                k = c.ff_kernel
                drop = ops.G8_DROP if (self.dropping and c.dropout_rate > 0) else 0
                keep = ops.gemm_8p_supported(M, c.ff, k * c.adim, k, ops.G8_BIAS_ACT | drop | ops.G8_KEEP_OUT) and \
                    ops.gemm_8p_supported(M, c.ff, k * c.adim, k, ops.G8_KEEP_IN | ops.G8_COLSUM)
                d1 = ops.gemm_8p_supported(M, c.adim, k * c.ff, k, 0) or ops.gemm_pn_supported(M, c.adim, k * c.ff, k, 0)
                # (no keep bits: the panel GEMM runs the data gradient of conv 2 on the transposed w_2 with the saved hidden
                #  activation as its ReLU' mask ...
                d2 = (not keep) and \
                    ops.gemm_pn_supported(M, c.ff, k * c.adim, k, ops.G8_SMASK | ops.G8_COLSUM)
                # ... or with a row-major keep image the forward conv writes from the 128-row kernel's epilogue: 4 bits per
                #  byte, 14 MB read in the place of the 110-MB activation at configs[1]; opt.ffn_keep4 off: the activation)
                keep4 = (not keep) and self.opt.ffn_keep4 and c.ff % 8 == 0 and \
                    ops.gemm_pn_supported(M, c.ff, k * c.adim, k, ops.G8_KEEP_IN | ops.G8_COLSUM)
                d2 = d2 or keep4
                if (keep or d2) and "w2" not in self._wt:
                    self._setup_wt("w2", (c.adim, k, c.ff))
                if d1 and "w1" not in self._wt:
                    self._setup_wt("w1", (c.ff, k, c.adim))
                keep, d1, d2 = keep and "w2" in self._wt, d1 and "w1" in self._wt, d2 and "w2" in self._wt
                keep4 = keep4 and d2
            self._ffn_plans[key] = (keep, d1, d2, keep4)
        return self._ffn_plans[key]

    def _lin_dgrad(self, dy, name, dx):
        """dx = dy W for the Linear weight `name` ([out][in]).  When the 384-column panel GEMM would take the k-contiguous form
        (in = 384 columns, opt.lin_dgrad_t off: never) it runs as dx = dy (W^T)^T on the transposed bf16 shadow of W."""
        suf = name.rsplit(".", 1)[1]
        M = dy.shape[0]
        key = (suf, M, dx.dtype, self._mode_tag, self.opt.lin_dgrad_t)
        if key not in self._lin_plans:
            use = False
            if self.bf16 and self.dev.type == "cuda" and self.opt.lin_dgrad_t:
                n_out, n_in = self.store.offsets[name][1]
                use = ops.gemm_pn_supported(M, n_in, n_out, 1, ops.G8_F32_OR_RES if dx.dtype == torch.float32 else 0)
                if use and suf not in self._wt:
                    self._setup_wt(suf, (n_out, 1, n_in))
                use = use and suf in self._wt and name in self._wt[suf][2]
            self._lin_plans[key] = use
        if self._lin_plans[key]:
            wt = self._wt[suf][2][name]
            ops.linear_fwd(dy, wt.view(wt.shape[0], wt.shape[2]), dx, compute=self.cmp)
        else:
            ops.linear_bwd_data(dy, self.W(name), dx, compute=self.cmp)

    def _act(self, name, shape):
        return self.ws.get(name, shape, self.adt)

    def _ln_fwd(self, tag, x, pre, eps=1e-12, out_dtype=None, lens=None, T=0):
        """lens (device int32 [B], rows of T frames): rows t >= lens[b] are stored as 0 -- the input of a k-tap convolution of a
        ragged batch (_check_ragged)."""
        p = self.store.p
        M, D = x.shape
        y = self.ws.get(tag + ".y", (M, D), out_dtype or self.adt)
        mean = self.ws.get(tag + ".mean", (M,))
        rstd = self.ws.get(tag + ".rstd", (M,))
        if lens is not None:
            ops.layernorm_fwd_ragged(x, p[pre + ".g"], p[pre + ".b"], y, mean, rstd, lens, M // T, T, eps)
        else:
            ops.layernorm_fwd(x, p[pre + ".g"], p[pre + ".b"], y, mean, rstd, eps)
        self.sv[tag] = (x, y, mean, rstd)
        return y

    def _ln_bwd(self, tag, dy, pre, dres, dx, dx16=None, nb=None, nxt=None):
        """nb = (bias-gradient view, scale) of the layer that produced the residual stream this LN read:
        its bias gradient is the column sum of dx; fused into the kernel on the bf16 path.
        nxt = dropout-site tag of that layer's output dropout (the next sub-layer of the backward schedule): with
        dropout on, the kernel also emits that sub-layer's masked bf16 gradient operand and masked bias gradient,
        which replaces the separate dropout_bwd_cast pass over g."""
        p, g = self.store.p, self.store.g
        x, _, mean, rstd = self.sv[tag]
        dropping = self.dropping and self.c.dropout_rate > 0
        if dropping and self.bf16 and self.opt.fuse_ln_dropout and nb is not None and nxt is not None and x.shape[1] % 128 == 0:
            dr = self._drop(self.c.dropout_rate, nxt)
            nx = (self._par + 1) % self._depth
            gm = self.ws.get(f"tmp.gm.{nx}", tuple(dx.shape), self.adt)
            ev = self._side_ev[nx]                     # side-stream readers of that scratch set must have drained
            if ev is not None:
                ev.wait_on(torch.cuda.current_stream())
                self._side_ev[nx] = None
            ops.layernorm_bwd(dy, x, p[pre + ".g"], mean, rstd, dres, dx, g[pre + ".g"], g[pre + ".b"], dx16=gm,
                              dxsum=nb[0], dxsum_scale=nb[1], drop=dr)
            self._gm_ready = nxt
            return
        if dropping and nxt is not None:
            nb = None          # a layer with output dropout: its bias gradient comes from the masked gradient (_gm)
        # (nxt is None: the layer has no output dropout -- the speech-embedding Linear -- and its bias gradient is the plain
        #  column sum of dx also when dropout is on; round 3: until then emb.b got no gradient in dropout-on steps)
        fuse = self.bf16 and nb is not None
        ops.layernorm_bwd(dy, x, p[pre + ".g"], mean, rstd, dres, dx, g[pre + ".g"], g[pre + ".b"], dx16=dx16,
                          dxsum=nb[0] if fuse else None, dxsum_scale=nb[1] if fuse else 1.0)
        if nb is not None and not fuse:
            self._bias_grad(dx, nb[0], nb[1])

    def _bias_grad(self, dy, gb, scale=1.0):
        ops.bias_grad(dy, gb, self.scratch64, scale)

    def _g16(self, g):
        """bf16 companion of the residual-stream gradient (written by the LayerNorm backward)."""
        return self.ws.get("grad.x16", tuple(g.shape), torch.bfloat16) if self.bf16 else None

    def _lin_wgrad(self, dy, x, dW):
        """Weight gradient of a Linear (dW += dy^T x), off the main stream.  bf16 path: the Linear weight gradients of a block
        (linear_out, linear_q/k/v, pointwise_conv2, pointwise_conv1 -- all reductions over the same tokens with 384 input
        channels) are collected and handed over as ONE grouped launch (ops.linear_bwd_weight_group): they feed nothing until the
        optimizer, their operands live in the scratch ring / the saved activations, and four of them fill the chip where each
        alone has 16-20 K-tiles per workgroup.  A3T_WGRAD_GROUP=0: one launch each."""
        if self._wg_group > 1:
            self._wg_pending.append((dy, x, dW, 1.0))
            self._wg_slots.add(self._par)       # the scratch set its operands may live in (tmp.gm / tmp.dg / tmp.dqkv of this sub-layer)
            if len(self._wg_pending) >= self._wg_group:
                self._wg_flush()
            return
        self._side(lambda: ops.linear_bwd_weight(dy, x, dW, compute=self.cmp))

    def _wg_flush(self):
        items, self._wg_pending = self._wg_pending, []
        slots, self._wg_slots = self._wg_slots, set()
        if items:
            cmp = self.cmp
            self._side(lambda: ops.linear_bwd_weight_group(items, compute=cmp))
            # A collected gradient may be handed over AFTER its sub-layer ended: the slot event _sub_end recorded then does
            # not cover this launch.  Re-record the event of every scratch set the group reads, behind the group (ADVICE r5:
            # with A3T_SIDE_DEPTH=8 the main stream could otherwise reuse tmp.gm.{slot} under the group kernel).
            if self.side is not None:
                for sl in slots:
                    ev = self._owned_event(("slot", sl))
                    ev.record(self.side)
                    self._side_ev[sl] = ev

    def _pre_ln(self, ga, g, g16):
        """The sub-layer's closing LayerNorm backward rewrites g / g16 in place: if the side-stream GEMMs read the
        gradient from there (no dropout copy), they must finish first."""
        if ga is g or ga is g16:
            self._wg_flush()              # (collected Linear weight gradients read the gradient in place too)
        if self.side is not None and (ga is g or ga is g16):
            torch.cuda.current_stream().wait_stream(self.side)

    # ------------------------------------------------------------------ FFN (MultiLayeredConv1d)
    def _ffn_fwd(self, tag, pre, x, T, lens=None):
        p, c = self.store.p, self.c
        M = x.shape[0]
        pad = (c.ff_kernel - 1) // 2
        if lens is not None and pad == 0:      # pointwise convs read no neighbour: nothing to zero
            lens = None
        y = self._ln_fwd(tag + ".ln", x, pre + ".ln", lens=lens, T=T)
        h = self._act(tag + ".h", (M, c.ff))
        keep, lay = None, 0
        if self._ffn_plan(M)[0]:  # one bit per element of h (value > 0 after relu / dropout) for the backward mask
            keep = self.ws.get(tag + ".keep", (ops.gemm_keep_bytes(M, c.ff),), torch.uint8)
        elif self._ffn_plan(M)[3]:      # the same bits as a row-major nibble image (128-row kernel -> panel kernel)
            keep, lay = self.ws.get(tag + ".keep4", (M * c.ff // 4,), torch.uint8), 1
        ops.conv_fwd(y, self.W(pre + ".w1"), h, T, pad, bias=p[pre + ".b1"], act=ACT_RELU, compute=self.cmp,
                     drop=self._drop(c.dropout_rate, tag + ".h"), keep_out=keep, keep_layout=lay)
        if lens is not None:      # the second conv's taps read zeros behind every row's length, not relu(b1 + ...)
            ops.zero_tail(h, lens, 1, M // T, T)
        xo = self.ws.get(tag + ".xo", (M, c.adim))
        ops.conv_fwd(h, self.W(pre + ".w2"), xo, T, pad, bias=p[pre + ".b2"], R=x, alpha=self._ffs, compute=self.cmp,
                     drop=self._drop(c.dropout_rate, tag + ".o"))
        self.sv[tag] = (y, h, keep, lay)
        return xo

    def _ffn_bwd(self, tag, pre, g, T, nb=None, nxt=None):
        """g = grad wrt the sub-layer output (fp32 residual stream, updated in place to the grad wrt
        the sub-layer input); in bf16 mode grad.x16 holds the same values in bf16 on entry and exit."""
        p, gr, c = self.store.p, self.store.g, self.c
        y, h, keep, lay = self.sv[tag]
        M = g.shape[0]
        pad = (c.ff_kernel - 1) // 2
        self._sub_begin()
        g16 = self._g16(g)
        ffs = self._ffs
        ga = self._gm(g, tag + ".o", c.dropout_rate, gr[pre + ".b2"], ffs)
        self._side(lambda: ops.conv_bwd_weight(ga, h, gr[pre + ".w2"], T, pad, alpha=ffs, compute=self.cmp))
        dh = self._act(self._t("tmp.dh"), (M, c.ff))
        # (without dropout b2's gradient = 0.5*colsum(g) was accumulated by the LayerNorm backward that
        #  produced g; the dropout on h folds into the relu mask S=h>0 and the 1/(1-p) factor)
        hd = self._drop(c.dropout_rate, tag + ".h")
        a_dh = ffs / (1.0 - hd[0]) if hd else ffs
        if keep is not None:     # k-contiguous conv of ga with the transposed weights, masked by the forward's keep bits
            ops.conv_fwd(ga, self._wt["w2"][2][pre + ".w2"], dh, T, c.ff_kernel - 1 - pad, alpha=a_dh, compute=self.cmp,
                         keep_in=keep, keep_layout=lay, colsum=gr[pre + ".b1"])
        elif self._ffn_plan(M)[2]:
            ops.conv_fwd(ga, self._wt["w2"][2][pre + ".w2"], dh, T, c.ff_kernel - 1 - pad, alpha=a_dh, compute=self.cmp,
                         S=h, colsum=gr[pre + ".b1"])
        else:
            ops.conv_bwd_data(ga, self.W(pre + ".w2"), dh, T, pad, S=h, alpha=a_dh,
                              compute=self.cmp, colsum=gr[pre + ".b1"] if self.bf16 else None)
        self._side(lambda: ops.conv_bwd_weight(dh, y, gr[pre + ".w1"], T, pad, compute=self.cmp))
        dy = self._act("tmp.dy", (M, c.adim))
        if self._ffn_plan(M)[1]:
            ops.conv_fwd(dh, self._wt["w1"][2][pre + ".w1"], dy, T, c.ff_kernel - 1 - pad, compute=self.cmp)
        else:
            ops.conv_bwd_data(dh, self.W(pre + ".w1"), dy, T, pad, compute=self.cmp)
        if not self.bf16:
            self._bias_grad(dh, gr[pre + ".b1"])
        self._pre_ln(ga, g, g16)
        self._ln_bwd(tag + ".ln", dy, pre + ".ln", g, g, g16, nb, nxt)
        self._sub_end()
        return g

    # ------------------------------------------------------------------ rel-pos self-attention
    def _mha_fwd(self, tag, pre, x, pos, keymask, B, T, lens=None, pos_rows=None):
        """LayerNorm, qkv and the positional rows; then one of three routes from (q, k, v, P) to ctx -- "fwd" (a3t_attn_fwd, keeps
        nothing for a backward), "train" (a3t_attn_fwd_train) or "mat" (materialised scores) -- and the output projection."""
        p, c = self.store.p, self.c
        d, dk = c.adim, c.dk
        M = B * T
        cmp = self.cmp
        y = self._ln_fwd(tag + ".ln", x, pre + ".ln")
        qkv = self._act(tag + ".qkv", (M, 3 * d))
        ops.linear_fwd(y, self.W(pre + ".wqkv"), qkv, bias=p[pre + ".bqkv"], compute=cmp)
        # q + pos_bias_u / q + pos_bias_v (attention.py:190-194): the fused kernels add the biases as they load their query
        # fragments (bit for bit what a3t_add_pos_bias stores); the two [M][d] tensors only exist for the materialised forward and,
        # in the backward, as operands of the dK / d linear_pos products (made there, off the main stream)
        # lens (a ragged batch, _check_ragged: fp32, eval mode, forward only) takes the materialised forward with the key mask
        # j < lens[b] and the legacy rel_shift taken at lens[b] (a3t_relpos_softmax_fwd_ragged).  P = linear_pos(pe[:T]) serves every
        # row: its first n rows are pe[:n] projected.  Query rows behind a row's length come out as 0 from the softmax, so the
        # probs @ V product and what follows stay finite there; no valid row reads them.
        # pos_rows = (slens, tlens, Tm, Tp), with lens = slens + tlens (packed rows, forward(lens=)): row b's table is
        # cat(pe[:sl_b], pe[:tl_b]), no prefix of one table.  linear_pos has no bias and works row by row, so
        # pos = pe[:max(Tm, Tp)] is projected once and a3t_concat_rows_ragged gathers the projected rows per batch row; the
        # position-score GEMM then reads a B operand of its own per row.
        ragged = lens is not None
        fused = (self._fused_now or self._fused_train_now) and ops.attn_fused_supported(dk, T) and not ragged
        pbias = (p[pre + ".u"], p[pre + ".v"])
        qu = qv = None
        if not fused:
            qu = self._act(tag + ".qu", (M, d))
            qv = self._act(tag + ".qv", (M, d))
            ops.add_pos_bias(qkv, pbias[0], pbias[1], qu, qv)
        P = None if ragged else self._P_ahead.get(tag)
        if P is not None:       # projected ahead on the side stream (by the model's forward)
            ev = self._pos_ev.get(tag[:3]) if self._pos_ev else None
            if ev is not None:
                ev.wait_on(torch.cuda.current_stream())
                self._pos_ev[tag[:3]] = None
        elif pos_rows is not None:
            Pt = self._act(tag + ".Pt", (pos.shape[0], d))
            ops.linear_fwd(pos, self.W(pre + ".wpos"), Pt, compute=cmp)
            P = self._act(tag + ".Prow", (M, d))
            ops.concat_rows_ragged(Pt, Pt, P, pos_rows[0], pos_rows[1], B, pos_rows[2], pos_rows[3], d, 0, 0)
        else:
            P = self._act(tag + ".P", (T, d))
            ops.linear_fwd(pos, self.W(pre + ".wpos"), P, compute=cmp)
        route = "fwd" if (self._fused_now and fused) else "train" if (self._fused_train_now and fused) else "mat"
        self.attn_path[tag[:-4]] = route
        self.block_dims[tag[:-4]] = (B, T)
        for k in (".fused", ".rs", ".signed"):      # the markers of an earlier pass under this tag
            self.sv.pop(tag + k, None)
        ctx = self._act(tag + ".ctx", (M, d))
        q = (qu, qv, qkv, P, keymask, ctx)
        if route == "mat":
            kept = self._attn_fwd_mat(tag, q, B, T, lens, pos_rows is not None)
        else:
            kept = (self._attn_fwd_only if route == "fwd" else self._attn_fwd_train)(tag, q, pbias, B, T)
        xo = self.ws.get(tag + ".xo", (M, d))
        ops.linear_fwd(ctx, self.W(pre + ".wo"), xo, bias=p[pre + ".bo"], R=x, compute=cmp,
                       drop=self._drop(c.dropout_rate, tag + ".o"))
        # (a forward-only or ragged pass keeps nothing for a backward)
        self.sv[tag] = None if kept is None else (y, qkv, qu, qv, P, kept[0], ctx, pos, kept[1])
        return xo

    def _attn_fwd_only(self, tag, q, pbias, B, T):
        c = self.c
        lse = self.ws.get(tag + ".lse", (B, c.heads, T))
        ops.attn_fwd(*q, lse, B, c.heads, T, 1.0 / math.sqrt(c.dk), drop=self._drop(c.attention_dropout_rate, tag + ".att") or (0.0, 0),
                     pos_bias=pbias if q[0] is None else None)
        self.sv[tag + ".fused"] = True      # (and nothing kept: returns None)

    def _attn_fwd_train(self, tag, q, pbias, B, T):
        """Fused forward, materialised backward: the saved probabilities stay un-normalised (1 / row sum in `rs`)."""
        c, H = self.c, self.c.heads
        adr = self._drop(c.attention_dropout_rate, tag + ".att")
        probs = self._act(tag + ".probs", (B, H, T, T))
        # attention dropout: ONE saved tensor -- the mask rides on the sign bits of probs (the score-gradient kernel and the dV
        # product read it there); the dropped copy only exists for the materialised score gradients (opt.attn_bwd_ds off)
        signed = bool(adr) and self.bf16 and self.opt.attn_bwd_ds and self.opt.attn_signed and T <= 2048     # (= the backward's ds_fused)
        pdrop = self._act(tag + ".pdrop", (B, H, T, T)) if adr and not signed else None
        lse = self.ws.get(tag + ".lse", (B, H, T))
        rs = self.ws.get(tag + ".rs", (B, H, T))
        ops.attn_fwd_train(*q, lse, probs, pdrop, rs, B, H, T, 1.0 / math.sqrt(c.dk), drop=adr or (0.0, 0),
                           pos_bias=pbias if q[0] is None else None)
        self.sv[tag + ".signed"] = signed
        self.sv[tag + ".rs"] = rs
        return probs, pdrop

    def _attn_fwd_mat(self, tag, q, B, T, lens, pos_per_row):
        c, H, d, dk, cmp = self.c, self.c.heads, self.c.adim, self.c.dk, self.cmp
        qu, qv, qkv, P, keymask, ctx = q
        # score-sized scratch: fp32 in fp32 mode; bf16 logits (fp32 softmax math) in bf16 mode
        sdt = torch.bfloat16 if self.bf16 else torch.float32
        ac = self.ws.get("tmp.ac", (B, H, T, T), sdt)
        bd = self.ws.get("tmp.bd", (B, H, T, T), sdt)
        kk = qkv.view(-1)[d:]
        vv = qkv.view(-1)[2 * d:]
        # ac[b,h] = (q+u) k^T ; bd[b,h] = (q+v) P_h^T   (attention.py:190-203)
        ops.gemm(qu, kk, ac, T, T, dk, d, 1, 3 * d, 1, T, batch=B * H, batch_inner=H, a_bs=(T * d, dk),
                 b_bs=(T * 3 * d, dk), c_bs=(H * T * T, T * T), compute=cmp)
        ops.gemm(qv, P, bd, T, T, dk, d, 1, d, 1, T, batch=B * H, batch_inner=H, a_bs=(T * d, dk),
                 b_bs=(T * d if pos_per_row else 0, dk), c_bs=(H * T * T, T * T), compute=cmp)
        probs = self._act(tag + ".probs", (B, H, T, T))
        adr = self._drop(c.attention_dropout_rate, tag + ".att")      # (None in eval mode, so with lens)
        pdrop = self._act(tag + ".pdrop", (B, H, T, T)) if adr else None
        if lens is not None:
            ops.relpos_softmax_fwd_ragged(ac, bd, lens, probs, B, H, T, 1.0 / math.sqrt(dk))
        else:
            ops.relpos_softmax_fwd(ac, bd, keymask, probs, B, H, T, 1.0 / math.sqrt(dk), probs_drop=pdrop,
                                   drop=adr or (0.0, 0))
        # ctx[b,:,h,:] = dropout(probs[b,h]) V[b,h]
        ops.gemm(pdrop if adr else probs, vv, ctx, T, dk, T, T, 1, 1, 3 * d, d, batch=B * H, batch_inner=H,
                 a_bs=(H * T * T, T * T), b_bs=(T * 3 * d, dk), c_bs=(T * d, dk), compute=cmp)
        return None if lens is not None else (probs, pdrop)

    def _mha_bwd(self, tag, pre, g, B, T, nb=None, nxt=None):
        p, gr, c = self.store.p, self.store.g, self.c
        d, H, dk = c.adim, c.heads, c.dk
        M = B * T
        cmp = self.cmp
        y, qkv, qu, qv, P, probs, ctx, pos, pdrop = self.sv[tag]
        scale = 1.0 / math.sqrt(dk)
        self._sub_begin()
        g16 = self._g16(g)
        ga = self._gm(g, tag + ".o", c.dropout_rate, gr[pre + ".bo"], 1.0)
        self._lin_wgrad(ga, ctx, gr[pre + ".wo"])
        dctx = self._act("tmp.dctx", (M, d))
        self._lin_dgrad(ga, pre + ".wo", dctx)
        kk = qkv.view(-1)[d:]
        vv = qkv.view(-1)[2 * d:]
        dqkv = self._act(self._t("tmp.dqkv"), (M, 3 * d))
        dkk = dqkv.view(-1)[d:]
        dvv = dqkv.view(-1)[2 * d:]
        sdt = torch.bfloat16 if self.bf16 else torch.float32
        rs = self.sv.get(tag + ".rs")      # fused training forward: probs / pdrop are exp(s - m_ref), rs = 1 / row sum
        dctx_v = dctx
        if rs is not None:                 # dV = pdrop^T (rs * dctx): fold the row normalisation into the small operand
            dctx_v = self._act(self._t("tmp.dctxs"), (M, d))      # (scaled on the side stream, in front of the one GEMM that reads it)
        signed = bool(self.sv.get(tag + ".signed"))      # the forward saved ONE tensor: |probs| = the probability, sign = dropped
        adr = self._drop(c.attention_dropout_rate, tag + ".att") if (pdrop is not None or signed) else None
        # bf16 path: the attention-dropout mask comes back from the counter RNG (same key and index as the forward) instead
        # of being read off the dropped probabilities: one T x T read less in the most HBM-bound kernel of the step
        regen = self.bf16 and adr is not None and T % 8 == 0 and T <= 2048
        # saved un-normalised probabilities + counter-RNG mask: dS / dBD in one launch, dprobs never stored (a3t_attn_bwd_ds)
        ds_fused = (rs is not None and self.bf16 and self.opt.attn_bwd_ds and (adr is None or regen) and dk % 32 == 0 and dk <= 192
                    and dk != 160 and T % 8 == 0)
        zb = (H * T * T, T * T)
        assert ds_fused or not signed
        if not ds_fused:
            dpr = self.ws.get("tmp.ac", (B, H, T, T), sdt)      # reuse the score buffers
            # dprobs[b,h] = dctx[b,:,h,:] V[b,h]^T
            ops.gemm(dctx, vv, dpr, T, T, dk, d, 1, 3 * d, 1, T, batch=B * H, batch_inner=H, a_bs=(T * d, dk),
                     b_bs=(T * 3 * d, dk), c_bs=zb, compute=cmp)
        # dV[b,h] = probs[b,h]^T dctx[b,:,h,:]
        fz = self.bf16   # bias / pos-bias gradients ride on the GEMM epilogues as column sums
        gbq = gr[pre + ".bqkv"]
        # The four N = d_k GEMMs below run as ONE round of co-resident tiles that all finish together: 576 atomics per
        # bias column in one burst cost ~40 us per GEMM.  Their column sums are therefore spread over S accumulator
        # copies (slot = (row tile + utterance) % S; arena slot, zeroed once per backward) and folded by one small kernel.
        S = self.colsum_slots
        sl = self._arena_slot("bwd32", tag + ".bsl", S * 4 * d) if fz else None
        csk = dict(colsum_bs1=dk, colsum_slots=S, colsum_ss=4 * d)
        # (independent of the dprobs -> softmax-backward chain: runs beside it on the side stream)
        make_q = qu is None        # fused forward: (q+u), (q+v) were never stored -- the dK product (second side stream, below) and
        if make_q:                 # the gradient of linear_pos (first side stream) read them: made on the second side stream
            qu = self._act("tmp.qu", (M, d))                  # (read on that stream only, in order)
            qv = self._act(self._t("tmp.qv"), (M, d))         # (read by the other side stream, whenever it gets there)

        def dv_gemm():
            if rs is not None:
                ops.attn_scale_rows(dctx, rs, dctx_v, B, H, T)
            ops.gemm(pdrop if pdrop is not None else probs, dctx_v, dvv, T, dk, T, 1, T, 1, d, 3 * d,
                     batch=B * H, batch_inner=H, a_bs=zb, b_bs=(T * d, dk), c_bs=(T * 3 * d, dk),
                     compute=cmp, colsum=sl[3 * d:] if fz else None, a_signmask=signed,
                     alpha=1.0 / (1.0 - adr[0]) if signed else 1.0, **csk)
            if make_q:      # behind dV (which does not read them): dK cannot start before the score gradients exist anyway
                ops.add_pos_bias(qkv, p[pre + ".u"], p[pre + ".v"], qu, qv)
        qv_ready = self._side(dv_gemm, want_event=make_q, urgent=True)
        zbd = zb
        # dq = ds K + dbd P as one launch of the streaming kernel where it runs (below); and the compact dBD matrix is not stored at all: it
        # is the flat dS sequence shifted by T - 1 elements, read by its two consumers as a strided VIEW of dS (row stride T + 1,
        # 2-byte aligned rows: the LDS-DMA takes them) with T zeros in front of every (b, h) block for the entries of its first row
        # that never reach the scores (attention.py:157-165).  A3T_ATTN_DBD_VIEW=0: the stored matrix.
        dual = ds_fused and fz and self.opt.attn_dq_dual and ops.gemm_tt_supported(T, dk, T, B * H)
        dview = ds_fused and fz and self.opt.attn_dbd_view
        if dview:
            bsv = T + T * T
            flat = self.ws.get(self._t("tmp.dsv"), (B * H * bsv,), torch.bfloat16, zero_once=True)
            ds, dbd = flat[T:], flat[1:]
            zbd = (H * bsv, bsv)       # (batch strides of ds and of its dbd view; zb stays the probabilities')
        elif self.bf16:
            ds = self.ws.get("tmp.ds16", (B, H, T, T), torch.bfloat16)
            dbd = self.ws.get(self._t("tmp.dbd16"), (B, H, T, T), torch.bfloat16)
        else:
            ds = dpr
            dbd = self.ws.get(self._t("tmp.dbd"), (B, H, T, T), sdt)
        if ds_fused:
            ops.attn_bwd_ds(dctx, ctx, qkv, probs, rs, ds, None if dview else dbd, B, H, T, scale, drop=adr or (0.0, 0),
                            signed_probs=signed, ds_bs=zbd[1] if dview else 0)
        else:
            ops.relpos_softmax_bwd(probs, dpr, ds, dbd, B, H, T, scale, probs_drop=None if regen else pdrop,
                                   drop_p=adr[0] if adr else 0.0, drop_key=adr[1] if regen else 0, rowscale=rs)
        # bf16 path, where a3t_attn_bwd_dpos takes the shape: its workspace is a scratch-ring tensor like tmp.qv (csrc/attn_dpos.hip)
        dpos = self.bf16 and dbd.dtype == torch.bfloat16 and ops.attn_bwd_dpos_plan(B, H, T, dk) is not None
        dpos_ws = self.ws.get(self._t("tmp.dPws"), (ops.attn_bwd_dpos_ws(B, H, T, dk),)) if dpos else None

        def pos_weight_grad():   # dP_h += sum_b dbd^T (q+v) -> d W_pos; only the side stream touches tmp.dP*
            if qv_ready is not None and self.side is not None:
                qv_ready.wait_on(self.side)
            if dpos:     # streaming product over groups of batch elements + a fold in fixed order: no atomics, no clear, no cast
                dP16 = self.ws.get("tmp.dP16", (T, d), torch.bfloat16)
                ops.attn_bwd_dpos(dbd, qv, dpos_ws, dP16, B, H, T, T + 1 if dview else T, zbd)
                ops.linear_bwd_weight(dP16, pos, gr[pre + ".wpos"], compute=cmp)
                return
            dP = self._arena_slot("bwd32", tag + ".dP", T * d).view(T, d)   # cleared once per backward (main stream)
            ops.gemm(dbd, qv, dP, T, dk, T, 1, T + 1 if dview else T, 1, d, d, batch=B * H, batch_inner=H, a_bs=zbd, b_bs=(T * d, dk),
                     c_bs=(0, dk), acc=ACC_ATOMIC, compute=cmp, a_view=dview)
            if self.bf16:
                dP16 = self.ws.get("tmp.dP16", (T, d), torch.bfloat16)
                ops.cast_bf16(dP, dP16)
                dP = dP16
            ops.linear_bwd_weight(dP, pos, gr[pre + ".wpos"], compute=cmp)
        self._side(pos_weight_grad)
        # bf16 path: dq = d(q+u) + d(q+v) goes straight into the q third of dqkv -- the first product stores, the second adds (sum
        # in fp32, one rounding); pos_bias_u / pos_bias_v / linear_q.bias take their gradients from the products' own column sums.
        # fp32 path: both products are kept (their plain column sums are the bias gradients) and added by a3t_add_pos_bias_bwd.
        dq_acc = fz
        dqu = dqkv if dq_acc else self._act("tmp.dqu", (M, d))
        dqv = dqkv if dq_acc else self._act("tmp.dqv", (M, d))
        ldq, cbq = (3 * d, (T * 3 * d, dk)) if dq_acc else (d, (T * d, dk))
        # dqu[b,h] = ds K ; dK[b,h] = ds^T (q+u)
        # bf16 path on the streaming kernel: dq = ds K + dbd P as ONE launch (two K loops into one accumulator set, one rounding, no
        # read-modify-write of the q third; their column sums come apart at the hand-over) -- A3T_ATTN_DQ_DUAL=0: two launches
        if dual:
            ops.gemm(ds, kk, dqkv, T, dk, T, T, 1, 1, 3 * d, ldq, batch=B * H, batch_inner=H, a_bs=zbd,
                     b_bs=(T * 3 * d, dk), c_bs=cbq, compute=cmp, colsum=sl,
                     second=(dbd, P, d, (0, dk), sl[d:]) + ((T + 1,) if dview else ()), **csk)
        else:
            ops.gemm(ds, kk, dqu, T, dk, T, T, 1, 1, 3 * d, ldq, batch=B * H, batch_inner=H, a_bs=zbd,
                     b_bs=(T * 3 * d, dk), c_bs=cbq, compute=cmp, colsum=sl if fz else None, **csk)
        dk_fn = lambda: ops.gemm(ds, qu, dkk, T, dk, T, 1, T, 1, d, 3 * d, batch=B * H, batch_inner=H,
                                 a_bs=zbd, b_bs=(T * d, dk), c_bs=(T * 3 * d, dk), compute=cmp,
                                 colsum=sl[2 * d:] if fz else None, **csk)
        if self.opt.attn_dk_main and dual and self.side is not None and make_q and qv_ready is not None:
            # dK on the MAIN queue behind dq where the products run on the streaming kernel (second session): they take turns on the
            # CUs whatever queue they sit on (128 KiB of LDS each), and a hand-over event behind the last of them cost the main queue
            # ~25 us of bubble per layer (profiles/r06_trace_attn_layer.txt): 39.52 / 39.56 -> 39.41 / 39.39 ms.  On the 128-row kernel
            # (configs[3]) dK and dq do run side by side: 58.2 -> 58.6 ms with dK on the main queue, so it stays on the side queue
            # there.  (q + u) and dV come from the second side queue: its event is long past here.
            qv_ready.wait_on(torch.cuda.current_stream())
            dk_fn()
            dk_done = None
        else:
            dk_done = self._side(dk_fn, want_event=True, urgent=True)
        # dqv[b,h] = dbd P_h ; dP_h += sum_b dbd^T (q+v)
        if not dual:
            ops.gemm(dbd, P, dqv, T, dk, T, T + 1 if dview else T, 1, 1, d, ldq, batch=B * H, batch_inner=H, a_bs=zbd, b_bs=(0, dk),
                     c_bs=cbq, acc=ACC_ADD if dq_acc else ACC_STORE, compute=cmp, colsum=sl[d:] if fz else None, a_view=dview, **csk)
        if not dq_acc:
            ops.add_pos_bias_bwd(dqu, dqv, dqkv)      # (the dq slice only)
        if dk_done is not None:      # the dV / dK slices of dqkv and their column sums come from the side stream
            dk_done.wait_on(torch.cuda.current_stream())
        if fz:   # d u, d v, d b_q = d u + d v, d b_k, d b_v from the slot sums (all four GEMMs have drained here); feeds nothing
            self._side(
                lambda: ops.attn_bias_fold(sl, S, d, gr[pre + ".u"], gr[pre + ".v"], gbq))       # but the optimizer
        else:
            self._bias_grad(dqu, gr[pre + ".u"])
            self._bias_grad(dqv, gr[pre + ".v"])
            self._bias_grad(dqkv, gbq)
        self._lin_wgrad(dqkv, y, gr[pre + ".wqkv"])
        dy = self._act("tmp.dy", (M, d))
        self._lin_dgrad(dqkv, pre + ".wqkv", dy)
        self._pre_ln(ga, g, g16)
        self._ln_bwd(tag + ".ln", dy, pre + ".ln", g, g, g16, nb, nxt)
        self._sub_end()
        return g

    # ------------------------------------------------------------------ convolution module
    def _bn_fwd(self, tag, z, pre, bufpre, act, out):
        p, b = self.store.p, self.store.buf
        M, C = z.shape
        stats = self._arena_slot("fwd64", tag + ".stats", 2 * C)      # cleared once per forward
        if self.training:
            ops.col_reduce(z, stats[:C], stats[C:], mode=1)
        mean = self.ws.get(tag + ".bnmean", (C,))
        rstd = self.ws.get(tag + ".bnrstd", (C,))
        ops.bn_act_fwd(z, stats, p[pre + ".g"], p[pre + ".b"], b[bufpre + ".rm"], b[bufpre + ".rv"], mean, rstd, out,
                       1e-5, self.bn_momentum if self.training else 0.0, self.training, act)
        if self.training:
            self.store.nbt[bufpre] = self.store.nbt.get(bufpre, 0) + 1
        self.sv[tag + ".bn"] = (z, mean, rstd)

    def _bn_bwd(self, tag, dy, pre, act, dz):
        p, gr = self.store.p, self.store.g
        z, mean, rstd = self.sv[tag + ".bn"]
        M, C = z.shape
        sums = self._arena_slot("bwd64", tag + ".bnsums", 2 * C)      # cleared once per backward
        ops.bn_act_bwd(dy, z, mean, rstd, p[pre + ".g"], p[pre + ".b"], sums, dz, gr[pre + ".g"], gr[pre + ".b"],
                       self.training, act, zero=False)

    def _conv_fwd(self, tag, pre, x, T, lens=None):
        p, c = self.store.p, self.c
        M, d = x.shape
        cmp = self.cmp
        y = self._ln_fwd(tag + ".ln", x, pre + ".ln")
        g2 = self._act(tag + ".g", (M, 2 * d))
        ops.linear_fwd(y, self.W(pre + ".pw1"), g2, bias=p[pre + ".pb1"], compute=cmp)
        glu = self._act(tag + ".glu", (M, d))
        z = self.ws.get(tag + ".z", (M, d))
        if lens is not None:
            ops.glu_dwconv_fwd_ragged(g2, p[pre + ".dw"], p[pre + ".db"], glu, z, lens, M // T, T)
        else:
            ops.glu_dwconv_fwd(g2, p[pre + ".dw"], p[pre + ".db"], glu, z, T)
        s = self._act(tag + ".s", (M, d))
        self._bn_fwd(tag, z, pre + ".bn", pre + ".bn", ACT_SWISH, s)
        xo = self.ws.get(tag + ".xo", (M, d))
        ops.linear_fwd(s, self.W(pre + ".pw2"), xo, bias=p[pre + ".pb2"], R=x, compute=cmp,
                       drop=self._drop(c.dropout_rate, tag + ".o"))
        self.sv[tag] = (y, g2, glu, s)
        return xo

    def _conv_bwd(self, tag, pre, g, T, nb=None, nxt=None):
        p, gr, c = self.store.p, self.store.g, self.c
        M, d = g.shape
        cmp = self.cmp
        y, g2, glu, s = self.sv[tag]
        self._sub_begin()
        g16 = self._g16(g)
        ga = self._gm(g, tag + ".o", c.dropout_rate, gr[pre + ".pb2"], 1.0)
        self._lin_wgrad(ga, s, gr[pre + ".pw2"])
        ds = self.ws.get("tmp.ds", (M, d))
        self._lin_dgrad(ga, pre + ".pw2", ds)
        dz = self.ws.get("tmp.dz", (M, d))
        self._bn_bwd(tag, ds, pre + ".bn", ACT_SWISH, dz)
        dg = self._act(self._t("tmp.dg"), (M, 2 * d))
        ops.glu_dwconv_bwd(dz, g2, glu, p[pre + ".dw"], dg, gr[pre + ".dw"], gr[pre + ".db"], T,
                           dgsum=gr[pre + ".pb1"])
        self._lin_wgrad(dg, y, gr[pre + ".pw1"])
        dy = self._act("tmp.dy", (M, d))
        self._lin_dgrad(dg, pre + ".pw1", dy)
        self._pre_ln(ga, g, g16)
        self._ln_bwd(tag + ".ln", dy, pre + ".ln", g, g, g16, nb, nxt)
        self._sub_end()
        return g

    # ------------------------------------------------------------------ one Conformer block
    def _check_ragged(self, lens, B):
        if self.bf16 or self.training or self._need_grad:
            raise ValueError("lens: ragged rows need an engine in fp32 compute, eval mode, forward only "
                             f"(compute={self.compute}: 'f32' and 'bf16x3' both count, training={self.training}, "
                             f"need_grad={self._need_grad})")
        if lens.dtype != torch.int32 or lens.numel() != B or lens.device.type != self.dev.type:
            raise ValueError(f"lens must be an int32 tensor of {B} entries on {self.dev}")

    def block_fwd(self, pre, x, pos, keymask, B, T, lens=None, pos_rows=None):
        """lens (device int32 [B]): the rows of the padded [B][T] batch have their own lengths and row b comes out as if it had
        been passed alone at lens[b]: keys j >= lens[b] are masked (keymask is not read), the legacy rel_shift is taken at
        lens[b], and every convolution with more than one tap reads zeros behind lens[b].  Rows behind a length hold finite
        values nobody reads.  fp32 compute, eval mode, forward only.  pos_rows: packed speech | text rows, see _mha_fwd."""
        # (encoder_layer.py:117-181)
        if lens is not None:
            self._check_ragged(lens, B)
        x = self._ffn_fwd(pre + ".ffm", pre + ".ffm", x, T, lens)
        x = self._mha_fwd(pre + ".mha", pre + ".mha", x, pos, keymask, B, T, lens, pos_rows)
        x = self._conv_fwd(pre + ".cnv", pre + ".cnv", x, T, lens)
        x = self._ffn_fwd(pre + ".ff", pre + ".ff", x, T, lens)
        return self._ln_fwd(pre + ".fin", x, pre + ".fin.ln", out_dtype=torch.float32)

    def block_bwd(self, pre, g, B, T):
        gr = self.store.g
        # every LayerNorm backward also delivers the bias gradient (and, with dropout, the masked gradient operand) of
        # the layer whose output it read = the next sub-layer of this schedule
        self._ln_bwd(pre + ".fin", g, pre + ".fin.ln", None, g, self._g16(g), (gr[pre + ".ff.b2"], 0.5), pre + ".ff.o")
        self._ffn_bwd(pre + ".ff", pre + ".ff", g, T, (gr[pre + ".cnv.pb2"], 1.0), pre + ".cnv.o")
        self._conv_bwd(pre + ".cnv", pre + ".cnv", g, T, (gr[pre + ".mha.bo"], 1.0), pre + ".mha.o")
        self._mha_bwd(pre + ".mha", pre + ".mha", g, B, T, (gr[pre + ".ffm.b2"], 0.5), pre + ".ffm.o")
        self._ffn_bwd(pre + ".ffm", pre + ".ffm", g, T, None)
        return g

    # ------------------------------------------------------------------ one transformer block (plain attention, absolute positions)
    def _tmha_fwd(self, tag, pre, x, keymask, B, T):
        """MultiHeadedAttention (attention.py:64-122) behind its LayerNorm: scores q k^T * scale, no positional term -- no (q + u),
        (q + v), linear_pos or band.  The three routes of _mha_fwd, chosen the same way (_attn_choice, attn_fused_supported): "fwd" /
        "train" = the band-free instantiations of the fused kernels (a3t_attn_fwd_plain / a3t_attn_fwd_train_plain), "mat" =
        a3t_softmax_plain_fwd between the two batched GEMMs; q is read in place from the fused projection."""
        p, c = self.store.p, self.c
        d, dk, H, cmp = c.adim, c.dk, c.heads, self.cmp
        M = B * T
        y = self._ln_fwd(tag + ".ln", x, pre + ".ln")
        qkv = self._act(tag + ".qkv", (M, 3 * d))
        ops.linear_fwd(y, self.W(pre + ".wqkv"), qkv, bias=p[pre + ".bqkv"], compute=cmp)
        fused = (self._fused_now or self._fused_train_now) and ops.attn_fused_supported(dk, T)
        route = "fwd" if (self._fused_now and fused) else "train" if (self._fused_train_now and fused) else "mat"
        self.attn_path[tag[:-4]] = route
        self.block_dims[tag[:-4]] = (B, T)
        for k in (".rs", ".signed"):      # the markers of an earlier pass under this tag
            self.sv.pop(tag + k, None)
        scale = 1.0 / math.sqrt(dk)
        adr = self._drop(c.attention_dropout_rate, tag + ".att")
        ctx = self._act(tag + ".ctx", (M, d))
        probs = pdrop = None
        if route == "fwd":           # keeps nothing for a backward
            lse = self.ws.get(tag + ".lse", (B, H, T))
            ops.attn_fwd_plain(qkv, keymask, ctx, lse, B, H, T, scale, drop=adr or (0.0, 0))
        elif route == "train":       # un-normalised probabilities, 1 / row sum in rs, the dropout mask on their sign bits (_attn_fwd_train)
            probs = self._act(tag + ".probs", (B, H, T, T))
            signed = bool(adr) and self.opt.attn_bwd_ds and self.opt.attn_signed and T <= 2048
            pdrop = self._act(tag + ".pdrop", (B, H, T, T)) if adr and not signed else None
            lse = self.ws.get(tag + ".lse", (B, H, T))
            rs = self.ws.get(tag + ".rs", (B, H, T))
            ops.attn_fwd_train_plain(qkv, keymask, ctx, lse, probs, pdrop, rs, B, H, T, scale, drop=adr or (0.0, 0))
            self.sv[tag + ".signed"] = signed
            self.sv[tag + ".rs"] = rs
        else:
            sdt = torch.bfloat16 if self.bf16 else torch.float32
            ac = self.ws.get("tmp.ac", (B, H, T, T), sdt)
            kk = qkv.view(-1)[d:]
            vv = qkv.view(-1)[2 * d:]
            zb, qb = (H * T * T, T * T), (T * 3 * d, dk)
            ops.gemm(qkv, kk, ac, T, T, dk, 3 * d, 1, 3 * d, 1, T, batch=B * H, batch_inner=H, a_bs=qb, b_bs=qb, c_bs=zb, compute=cmp)
            probs = self._act(tag + ".probs", (B, H, T, T))
            pdrop = self._act(tag + ".pdrop", (B, H, T, T)) if adr else None
            ops.softmax_plain_fwd(ac, keymask, probs, B, H, T, scale, probs_drop=pdrop, drop=adr or (0.0, 0))
            ops.gemm(pdrop if adr else probs, vv, ctx, T, dk, T, T, 1, 1, 3 * d, d, batch=B * H, batch_inner=H, a_bs=zb, b_bs=qb,
                     c_bs=(T * d, dk), compute=cmp)
        xo = self.ws.get(tag + ".xo", (M, d))
        ops.linear_fwd(ctx, self.W(pre + ".wo"), xo, bias=p[pre + ".bo"], R=x, compute=cmp,
                       drop=self._drop(c.dropout_rate, tag + ".o"))
        self.sv[tag] = None if route == "fwd" else (y, qkv, probs, ctx, pdrop)
        return xo

    def _tmha_bwd(self, tag, pre, g, B, T, nb=None, nxt=None):
        """dS, then the three products around it: dq = dS K (one launch, no second operand pair), dK = dS^T q, dV = P^T dctx, all into
        the thirds of dqkv.  Behind the fused training forward dS comes from the saved un-normalised probabilities in one launch
        (a3t_attn_bwd_ds with dbd = NULL; dV reads the dropout mask off their sign bits), otherwise from the dprobs GEMM and
        a3t_softmax_plain_bwd.  No positional-bias column sums and no linear_pos gradient; the bias of the fused projection is the
        column sum of dqkv."""
        gr, c = self.store.g, self.c
        d, H, dk, cmp = c.adim, c.heads, c.dk, self.cmp
        M = B * T
        y, qkv, probs, ctx, pdrop = self.sv[tag]
        self._sub_begin()
        g16 = self._g16(g)
        ga = self._gm(g, tag + ".o", c.dropout_rate, gr[pre + ".bo"], 1.0)
        self._lin_wgrad(ga, ctx, gr[pre + ".wo"])
        dctx = self._act("tmp.dctx", (M, d))
        self._lin_dgrad(ga, pre + ".wo", dctx)
        kk = qkv.view(-1)[d:]
        vv = qkv.view(-1)[2 * d:]
        dqkv = self._act(self._t("tmp.dqkv"), (M, 3 * d))
        dkk = dqkv.view(-1)[d:]
        dvv = dqkv.view(-1)[2 * d:]
        sdt = torch.bfloat16 if self.bf16 else torch.float32
        zb, qb = (H * T * T, T * T), (T * 3 * d, dk)
        scale = 1.0 / math.sqrt(dk)
        rs = self.sv.get(tag + ".rs")      # fused training forward: probs / pdrop are exp(s - m_ref), rs = 1 / row sum
        signed = bool(self.sv.get(tag + ".signed"))      # ONE saved tensor: |probs| = the probability, sign = dropped
        adr = self._drop(c.attention_dropout_rate, tag + ".att") if (pdrop is not None or signed) else None
        regen = self.bf16 and adr is not None and T % 8 == 0 and T <= 2048      # the mask back from the counter RNG (_mha_bwd)
        ds_fused = rs is not None and self.opt.attn_bwd_ds and (adr is None or regen) and ops.attn_fused_supported(dk, T)
        assert ds_fused or not signed
        dctx_v = dctx
        if rs is not None:                 # dV = pdrop^T (rs * dctx): the row normalisation folded into the small operand
            dctx_v = self._act("tmp.dctxs", (M, d))
            ops.attn_scale_rows(dctx, rs, dctx_v, B, H, T)
        ops.gemm(pdrop if pdrop is not None else probs, dctx_v, dvv, T, dk, T, 1, T, 1, d, 3 * d, batch=B * H, batch_inner=H,
                 a_bs=zb, b_bs=(T * d, dk), c_bs=qb, compute=cmp, a_signmask=signed, alpha=1.0 / (1.0 - adr[0]) if signed else 1.0)
        ds = self.ws.get("tmp.ds16", (B, H, T, T), torch.bfloat16) if self.bf16 else None
        if ds_fused:
            ops.attn_bwd_ds(dctx, ctx, qkv, probs, rs, ds, None, B, H, T, scale, drop=adr or (0.0, 0), signed_probs=signed)
        else:
            dpr = self.ws.get("tmp.ac", (B, H, T, T), sdt)      # (the score buffer of the forward)
            ops.gemm(dctx, vv, dpr, T, T, dk, d, 1, 3 * d, 1, T, batch=B * H, batch_inner=H, a_bs=(T * d, dk), b_bs=qb, c_bs=zb,
                     compute=cmp)
            if ds is None:
                ds = dpr                                        # (fp32: in place)
            ops.softmax_plain_bwd(probs, dpr, ds, B, H, T, scale, probs_drop=None if regen else pdrop,
                                  drop_p=adr[0] if adr else 0.0, drop_key=adr[1] if regen else 0, rowscale=rs)
        ops.gemm(ds, kk, dqkv, T, dk, T, T, 1, 1, 3 * d, 3 * d, batch=B * H, batch_inner=H, a_bs=zb, b_bs=qb, c_bs=qb, compute=cmp)
        ops.gemm(ds, qkv, dkk, T, dk, T, 1, T, 1, 3 * d, 3 * d, batch=B * H, batch_inner=H, a_bs=zb, b_bs=qb, c_bs=qb, compute=cmp)
        self._bias_grad(dqkv, gr[pre + ".bqkv"])
        self._lin_wgrad(dqkv, y, gr[pre + ".wqkv"])
        dy = self._act("tmp.dy", (M, d))
        self._lin_dgrad(dqkv, pre + ".wqkv", dy)
        self._pre_ln(ga, g, g16)
        self._ln_bwd(tag + ".ln", dy, pre + ".ln", g, g, g16, nb, nxt)
        self._sub_end()
        return g

    def tblock_fwd(self, pre, x, keymask, B, T):
        """x += drop(out(attn(ln1 x))); x += drop(ffn(ln2 x))  (transformer/encoder_layer.py:62-121, normalize_before, no
        concat_after); no LayerNorm closes the block."""
        x = self._tmha_fwd(pre + ".mha", pre + ".mha", x, keymask, B, T)
        return self._ffn_fwd(pre + ".ff", pre + ".ff", x, T)

    def tblock_bwd(self, pre, g, B, T, prev=None):
        """prev: the block in front of this one in the same stack (None for the first) -- its FFN wrote the residual stream this
        block's first LayerNorm read, so that LayerNorm's backward delivers prev.ff.b2's gradient (block_bwd)."""
        gr = self.store.g
        self._ffn_bwd(pre + ".ff", pre + ".ff", g, T, (gr[pre + ".mha.bo"], 1.0), pre + ".mha.o")
        self._tmha_bwd(pre + ".mha", pre + ".mha", g, B, T, (gr[prev + ".ff.b2"], 1.0) if prev else None,
                       prev + ".ff.o" if prev else None)
        return g

    def _attn_choice(self, B, T, need_grad):
        """(forward-only fused, fused training forward) for the blocks that run at T tokens per utterance: decided once per
        forward() and block shape.  The backward follows what the forward saved under the block's tag."""
        nblk = B * self.c.heads * ((T + 127) // 128)
        fused_now = (self.fused_attn_fwd_only and not need_grad) or \
            (self.fused_attn_auto and not need_grad and nblk >= 64)
        fused_train_now = self.fused_attn_train and need_grad and not fused_now and \
            self.fused_attn_train_min <= nblk <= 65536 and T <= 2048
        return fused_now, fused_train_now
