"""Thin host wrappers over the C ABI (include/a3t_hip.h): torch tensors supply device memory and
the current HIP stream, every computation happens in liba3t_hip.so.  No torch math here."""
import ctypes
import os

import torch

from . import _lib as L
from ._lib import ACC_ADD, ACC_ATOMIC, ACC_SOLE, ACC_STORE, ACT_NONE, ACT_RELU, ACT_SWISH, ACT_TANH, BF16, F32

__all__ = ["gemm", "gemm_plan", "linear_fwd", "linear_bwd_data", "linear_bwd_weight", "conv_fwd", "conv_bwd_data",
           "conv_bwd_weight"]


# bench.py sets PROFILE = [] to bracket every GEMM launch with HIP events on the launch stream:
# entries are (kernel name as rocprofv3 prints it, algorithmic FLOPs of the launch, start, end).
PROFILE = None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _gemm_desc(A, B, C, M, N, K, a_rs, a_cs, b_rs, b_cs, c_rs, *, b_ts=0, bias=None, R=None, S=None, batch=1,
               batch_inner=1, a_bs=(0, 0), b_bs=(0, 0), c_bs=(0, 0), taps=1, pad=0, dil=1, Tseq=0, kshift=0, alpha=1.0,
               act=ACT_NONE, acc=ACC_STORE, splitk=1, compute=F32, colsum=None, colsum_bs1=0, colsum_scale=1.0,
               drop=None, colsum_slots=1, colsum_ss=0, keep_out=None, keep_in=None, a_signmask=False, keep_layout=0, second=None,
               a_view=False):
    """The a3t_gemm_desc of C (op)= alpha*mask(act(A(m,k) B(n,k) + bias)) + R  -- see include/a3t_hip.h."""
    d = L.GemmDesc()
    d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), C.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.R = R.data_ptr() if R is not None else None
    d.S = S.data_ptr() if S is not None else None
    d.M, d.N, d.K = M, N, K
    d.a_rs, d.a_cs, d.b_rs, d.b_cs, d.b_ts, d.c_rs = a_rs, a_cs, b_rs, b_cs, b_ts, c_rs
    d.batch, d.batch_inner = batch, batch_inner
    d.a_bs0, d.a_bs1 = a_bs
    d.b_bs0, d.b_bs1 = b_bs
    d.c_bs0, d.c_bs1 = c_bs
    d.taps, d.pad, d.dil, d.Tseq, d.kshift = taps, pad, dil, Tseq, kshift
    d.alpha, d.act, d.accumulate, d.splitk = alpha, act, acc, splitk
    d.a_dtype, d.b_dtype, d.c_dtype, d.compute = _dt(A), _dt(B), _dt(C), compute
    d.s_dtype = _dt(S) if S is not None else F32
    d.colsum = colsum.data_ptr() if colsum is not None else None
    d.colsum_bs1, d.colsum_scale = colsum_bs1, colsum_scale
    d.colsum_slots, d.colsum_ss = colsum_slots, colsum_ss
    d.drop_p, d.drop_key = (drop if drop is not None else (0.0, 0))
    d.keep_out = keep_out.data_ptr() if keep_out is not None else None
    d.keep_in = keep_in.data_ptr() if keep_in is not None else None
    d.a_signmask = 1 if a_signmask else 0
    d.keep_layout = keep_layout
    d.a_unaligned = 1 if a_view else 0      # A is a 2-byte aligned strided view (the compact dBD read off dS)
    if second is not None:      # (A2, B2, b2_cs, (b2_bs0, b2_bs1), colsum2[, a2_rs]): C = alpha (A B + A2 B2) in one launch of the
        A2, B2, b2_cs, b2_bs, cs2 = second[:5]      # streaming kernel; a2_rs given: A2 is such a view with that row stride
        d.A2, d.B2, d.b2_cs = A2.data_ptr(), B2.data_ptr(), b2_cs
        d.b2_bs0, d.b2_bs1 = b2_bs
        d.colsum2 = cs2.data_ptr() if cs2 is not None else None
        if len(second) > 5:
            d.a2_rs = second[5]
            d.a_unaligned |= 2
    return d


def gemm(*args, **kw):
    """C (op)= alpha*mask(act(A(m,k) B(n,k) + bias)) + R; arguments as _gemm_desc."""
    lib = L.load()
    d = _gemm_desc(*args, **kw)
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()          # torch's current stream == the stream handed to a3t_gemm
        L.check(lib.a3t_gemm(ctypes.byref(d), _stream()), "a3t_gemm")
        e1.record()
        PROFILE.append((lib.a3t_gemm_last_kernel().decode(), (4.0 if d.A2 else 2.0) * d.M * d.N * d.K * d.batch, e0, e1,
                        (d.M, d.N, d.K, d.batch, d.taps, d.splitk)))
        return
    L.check(lib.a3t_gemm(ctypes.byref(d), _stream()), "a3t_gemm")


def gemm_plan(*args, **kw):
    """Name of the kernel gemm(*args, **kw) would launch (as a3t_gemm_last_kernel reports it), or None where a3t_gemm would
    reject the descriptor.  Host code only (a3t_gemm_plan): nothing runs and no tensor is read, so they may live on the CPU."""
    name = ctypes.create_string_buffer(128)
    rc = L.load().a3t_gemm_plan(ctypes.byref(_gemm_desc(*args, **kw)), name, len(name))
    return name.value.decode() if rc == 0 else None


_SPLITK_TARGET = 1000      # workgroups of a split-K grid on the 128x128 kernel (500 / 700 / 1500 / 2000 measured in round 3: slower)


def _splitk_for(n_tiles, K, ktile=64):
    """Token-reduction GEMMs (weight gradients) have few output tiles: split K over workgroups so the
    grid is ONE resident wave of the kernel variant a3t_gemm will pick -- ~1000 workgroups for the
    single-buffer variant (4/CU, chosen when tiles*splitk >= 768), ~440 for the double-buffered one
    (2/CU); more splits only add fp32 atomics (measured on MI355X, tools/tn_bench*.py)."""
    target = _SPLITK_TARGET if n_tiles >= 64 else 440
    s = max(1, target // max(n_tiles, 1))
    s = min(s, max(1, K // (ktile * 8)))
    return int(s)


# ---- y = x W^T (+bias): torch.nn.Linear / 1x1 Conv1d -----------------------------------------
def linear_fwd(x, W, out, bias=None, R=None, alpha=1.0, act=ACT_NONE, compute=F32, drop=None):
    M, K = x.shape
    N = W.shape[0]
    gemm(x, W, out, M, N, K, K, 1, K, 1, N, bias=bias, R=R, alpha=alpha, act=act, compute=compute, drop=drop)


def linear_bwd_data(dy, W, dx, S=None, alpha=1.0, acc=ACC_STORE, compute=F32, colsum=None):
    """dx[M,K] = alpha * relu_mask_S(dy[M,N] @ W[N,K]);  colsum += column sums of dx"""
    M, N = dy.shape
    K = W.shape[1]
    gemm(dy, W, dx, M, K, N, N, 1, 1, K, K, S=S, alpha=alpha, acc=acc, compute=compute, colsum=colsum)


def linear_bwd_weight(dy, x, dW, alpha=1.0, compute=F32):
    """dW[N,K] += alpha * dy[M,N]^T @ x[M,K]   (reduction over tokens, split-K + fp32 atomics)"""
    M, N = dy.shape
    K = x.shape[1]
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    # ACC_SOLE: a parameter gradient has one writer at a time -- kernels that fold split-K partials need no atomics for it
    gemm(dy, x, dW, N, K, M, 1, N, 1, K, K, alpha=alpha, acc=ACC_SOLE, splitk=_splitk_for(tiles, M),
         compute=compute)


def linear_bwd_weight_group(items, compute=F32):
    """items = [(dy, x, dW, alpha), ...] over the same tokens: dW_i += alpha_i * dy_i^T @ x_i.  On the bf16 path all of them run
    as ONE launch of the 128 x 384-tile token-reduction kernel (a3t_gemm_tn3_group); when the library declines (fp32 compute,
    shapes outside the kernel's contract, kernel switched off) they are launched one by one."""
    if compute == BF16 and len(items) > 1 and len(items) <= 8:
        lib = L.load()
        arr = (L.GemmDesc * len(items))()
        for d, (dy, x, dW, alpha) in zip(arr, items):
            M, N = dy.shape
            K = x.shape[1]
            d.A, d.B, d.C = dy.data_ptr(), x.data_ptr(), dW.data_ptr()
            d.M, d.N, d.K = N, K, M
            d.a_rs, d.a_cs, d.b_rs, d.b_cs, d.b_ts, d.c_rs = 1, N, 1, K, 0, K
            d.batch, d.batch_inner, d.taps, d.dil = 1, 1, 1, 1
            d.alpha, d.act, d.accumulate, d.splitk = alpha, ACT_NONE, ACC_SOLE, 1
            d.a_dtype, d.b_dtype, d.c_dtype, d.compute, d.s_dtype = _dt(dy), _dt(x), _dt(dW), compute, F32
            d.colsum_slots = 1
        if PROFILE is not None:      # bench.py: one table row for the whole group
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        rc = lib.a3t_gemm_tn3_group(ctypes.cast(arr, ctypes.c_void_p), len(items), _stream())
        if rc == 0:
            if PROFILE is not None:
                e1.record()
                tok, cin = items[0][0].shape[0], items[0][1].shape[1]
                cout = sum(dy.shape[1] for dy, _, _, _ in items)
                PROFILE.append((lib.a3t_gemm_last_kernel().decode() + f" x{len(items)} grouped", 2.0 * tok * cout * cin, e0, e1,
                                (cout, cin, tok, 1, 1, 1)))
            return True
        if rc != -1:
            L.check(rc, "a3t_gemm_tn3_group")
    for dy, x, dW, alpha in items:
        linear_bwd_weight(dy, x, dW, alpha=alpha, compute=compute)
    return False


# ---- Conv1d over time as implicit-im2col GEMM; weights kept as Wk[N][taps][Cin] --------------
def conv_fwd(x, Wk, out, Tseq, pad, dil=1, bias=None, R=None, alpha=1.0, act=ACT_NONE, compute=F32, drop=None,
             keep_out=None, keep_in=None, colsum=None, S=None, keep_layout=0):
    M, Cin = x.shape
    N, taps, _ = Wk.shape
    gemm(x, Wk, out, M, N, taps * Cin, Cin, 1, taps * Cin, 1, N, b_ts=Cin, bias=bias, R=R, taps=taps, pad=pad,
         dil=dil, Tseq=Tseq, alpha=alpha, act=act, compute=compute, drop=drop, keep_out=keep_out, keep_in=keep_in,
         colsum=colsum, S=S, keep_layout=keep_layout)


G8_BIAS_ACT, G8_DROP, G8_KEEP_OUT, G8_KEEP_IN, G8_F32_OR_RES, G8_COLSUM, G8_SMASK = 1, 2, 4, 8, 16, 32, 64


def gemm_8p_supported(M, N, K, taps=1, flags=0):
    """True when a3t_gemm runs this k-contiguous bf16 problem, with the epilogue `flags`, on the persistent 8-phase kernel
    (csrc/gemm_bf16_8p.hip)."""
    return bool(L.load().a3t_gemm_8p_supported(int(M), int(N), int(K), int(taps), int(flags)))


def gemm_pn_supported(M, N, K, taps=1, flags=0):
    """True when a3t_gemm runs this k-contiguous bf16 problem on the 384-column panel kernel (csrc/gemm_bf16_pn.hip)."""
    return bool(L.load().a3t_gemm_pn_supported(int(M), int(N), int(K), int(taps), int(flags)))


def gemm_tt_supported(M, N, K, batch):
    """True when a3t_gemm runs the batched score-sized product on the streaming kernel (csrc/gemm_bf16_tt.hip) -- the precondition
    of gemm(second=...)."""
    return bool(L.load().a3t_gemm_tt_supported(int(M), int(N), int(K), int(batch)))


def gemm_mode_tag():
    """(8-phase mode, panel mode) the dispatcher's cost models currently run under -- part of every cached GEMM plan key."""
    lib = L.load()
    m8 = lib.a3t_gemm_8p_mode(2)
    lib.a3t_gemm_8p_mode(m8)
    mp = lib.a3t_gemm_pn_mode(2)
    lib.a3t_gemm_pn_mode(mp)
    return (m8, mp)


def collate_paint(fs, fe, alen, sel, mspan, nms, flen, tlen, masked, speech_mask, text_mask, sp, tp, sega_emb):
    B, P = fs.shape
    Tm, Tp, S = masked.shape[1], text_mask.shape[1], mspan.shape[1]
    L.check(L.load().a3t_collate_paint(_ptr(fs), _ptr(fe), _ptr(alen), _ptr(sel), _ptr(mspan), _ptr(nms), _ptr(flen), _ptr(tlen),
                                       _ptr(masked), _ptr(speech_mask), _ptr(text_mask), _ptr(sp), _ptr(tp), B, Tm, Tp, P, S,
                                       int(bool(sega_emb)), _stream()), "collate_paint")


def segment_colsum(x, out, B, T):
    L.check(L.load().a3t_segment_colsum(_ptr(x), _ptr(out), B, T, x.shape[1], _stream()), "segment_colsum")


def gemm_keep_bytes(M, N):
    return int(L.load().a3t_gemm_keep_bytes(int(M), int(N)))


def conv_bwd_data(dy, Wk, dx, Tseq, pad, dil=1, S=None, alpha=1.0, compute=F32, colsum=None):
    """dx[m][c] = sum_tap sum_n dy[m-(tap-pad)*dil][n] Wk[n][tap][c]: the same im2col loader on dy
    with the taps read back to front (pad' = taps-1-pad) and B addressed as W^T via strides."""
    M, N = dy.shape
    _, taps, Cin = Wk.shape
    Wv = Wk.view(-1)[(taps - 1) * Cin:]
    gemm(dy, Wv, dx, M, Cin, taps * N, N, 1, 1, taps * Cin, Cin, b_ts=-Cin, S=S, taps=taps, pad=taps - 1 - pad,
         dil=dil, Tseq=Tseq, alpha=alpha, compute=compute, colsum=colsum)


def conv_bwd_weight(dy, x, dWk, Tseq, pad, dil=1, alpha=1.0, compute=F32):
    """dWk[n][tap][c] += alpha * sum_m dy[m][n] x[m+(tap-pad)*dil][c]  (one token-shifted TN GEMM per tap)"""
    M, N = dy.shape
    Cin = x.shape[1]
    taps = dWk.shape[1]
    if compute == BF16 and dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and Cin % 128 == 0 \
            and N % 8 == 0 and taps > 1:
        # one launch: output columns (tap, c); every 128-column tile carries its own token shift
        tiles = ((N + 127) // 128) * (taps * Cin // 128)
        gemm(dy, x, dWk, N, taps * Cin, M, 1, N, 1, Cin, taps * Cin, taps=taps, pad=pad, dil=dil, Tseq=Tseq,
             alpha=alpha, acc=ACC_SOLE, splitk=_splitk_for(tiles, M), compute=compute)
        return
    tiles = ((N + 127) // 128) * ((Cin + 127) // 128)
    sk = _splitk_for(tiles, M)
    flat = dWk.view(-1)
    for tap in range(taps):
        gemm(dy, x, flat[tap * Cin:], N, Cin, M, 1, N, 1, Cin, taps * Cin, Tseq=Tseq, kshift=(tap - pad) * dil,
             alpha=alpha, acc=ACC_ATOMIC, splitk=sk, compute=compute)


# ---- row / column kernels --------------------------------------------------------------------
def _dto(t):
    return _dt(t) if t is not None else F32


def layernorm_fwd(x, g, b, y, mean, rstd, eps):
    M, D = x.shape
    L.check(L.load().a3t_layernorm_fwd(_ptr(x), _ptr(g), _ptr(b), _ptr(y), _dt(y), _ptr(mean), _ptr(rstd), M, D, eps,
                                       _stream()), "ln_fwd")


def layernorm_bwd(dy, x, g, mean, rstd, dres, dx, dg, db, dx16=None, dxsum=None, dxsum_scale=1.0, drop=(0.0, 0)):
    """drop=(p, key): dx16 / dxsum carry the dropout-masked gradient of the consumer sub-layer's branch."""
    M, D = x.shape
    L.check(L.load().a3t_layernorm_bwd(_ptr(dy), _dt(dy), _ptr(x), _ptr(g), _ptr(mean), _ptr(rstd), _ptr(dres),
                                       _ptr(dx), _ptr(dx16), _ptr(dg), _ptr(db), _ptr(dxsum), dxsum_scale, M, D,
                                       drop[0], drop[1], _stream()), "ln_bwd")


def col_reduce(x, out0, out1=None, y=None, rowmask=None, mode=0, ld=None):
    M, C = x.shape
    L.check(L.load().a3t_col_reduce(_ptr(x), _dt(x), _ptr(y), _ptr(rowmask), _ptr(out0), _ptr(out1), M, C,
                                    ld if ld is not None else x.stride(0), mode, _stream()), "col_reduce")


def f64_to_f32_add(src, dst, scale=1.0):
    L.check(L.load().a3t_f64_to_f32_add(_ptr(src), _ptr(dst), dst.numel(), scale, _stream()), "f64_to_f32_add")


def bias_grad(dy, dbias, scratch64, scale=1.0):
    """dbias += scale * colsum(dy) via the double-precision column reducer."""
    n = dy.shape[1]
    s = scratch64[:n]
    s.zero_()
    col_reduce(dy, s, mode=0)
    f64_to_f32_add(s, dbias, scale)


def bn_act_fwd(z, stats, g, b, rmean, rvar, mean_out, rstd_out, y, eps, momentum, training, act):
    M, C = z.shape
    L.check(L.load().a3t_bn_act_fwd(_ptr(z), _ptr(stats), _ptr(g), _ptr(b), _ptr(rmean), _ptr(rvar), _ptr(mean_out),
                                    _ptr(rstd_out), _ptr(y), _dt(y), M, C, eps, momentum, int(training), act,
                                    _stream()), "bn_act_fwd")


def bn_act_bwd(dy, z, mean, rstd, g, b, sums, dz, dg, db, training, act, zero=True):
    M, C = z.shape
    lib = L.load()
    if zero:
        sums.zero_()
    L.check(lib.a3t_bn_act_bwd_a(_ptr(dy), _dt(dy), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(g), _ptr(b), _ptr(sums), M, C,
                                 act, _stream()), "bn_bwd_a")
    L.check(lib.a3t_bn_act_bwd_b(_ptr(dy), _dt(dy), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(g), _ptr(b), _ptr(sums),
                                 _ptr(dz), _ptr(dg), _ptr(db), M, C, int(training), act, _stream()), "bn_bwd_b")


def glu_dwconv_fwd(g, wdw, bdw, glu, z, Tseq):
    M, C = glu.shape
    L.check(L.load().a3t_glu_dwconv_fwd(_ptr(g), _dt(g), _ptr(wdw), _ptr(bdw), _ptr(glu), _dt(glu), _ptr(z), M, C,
                                        wdw.shape[1], Tseq, _stream()), "glu_dwconv_fwd")


def glu_dwconv_bwd(dz, g, glu, wdw, dg, dwdw, dbdw, Tseq, dgsum=None):
    M, C = glu.shape
    L.check(L.load().a3t_glu_dwconv_bwd(_ptr(dz), _ptr(g), _dt(g), _ptr(glu), _dt(glu), _ptr(wdw), _ptr(dg), _dt(dg),
                                        _ptr(dwdw), _ptr(dbdw), _ptr(dgsum), M, C, wdw.shape[1], Tseq, _stream()),
            "glu_dwconv_bwd")


def add_pos_bias(qkv, u, v, qu, qv):
    M, d = qu.shape
    L.check(L.load().a3t_add_pos_bias(_ptr(qkv), _ptr(u), _ptr(v), _ptr(qu), _ptr(qv), _dt(qkv), M, d, _stream()),
            "pos_bias")


def add_pos_bias_bwd(dqu, dqv, dqkv):
    M, d = dqu.shape
    L.check(L.load().a3t_add_pos_bias_bwd(_ptr(dqu), _ptr(dqv), _ptr(dqkv), _dt(dqu), M, d, _stream()),
            "pos_bias_bwd")


def relpos_softmax_fwd(ac, bd, keymask, probs, B, H, T, scale, probs_drop=None, drop=(0.0, 0)):
    L.check(L.load().a3t_relpos_softmax_fwd(_ptr(ac), _ptr(bd), _dt(ac), _ptr(keymask), _ptr(probs), _dt(probs), B, H, T,
                                            T * T, T * T, T * T, scale, _ptr(probs_drop), drop[0], drop[1],
                                            _stream()), "softmax_fwd")


def relpos_softmax_bwd(probs, dprobs, ds, dbd, B, H, T, scale, probs_drop=None, drop_p=0.0, dbd_head_major=False,
                       drop_key=0, rowscale=None):
    """ds/dbd share a dtype; ds may be dprobs itself (fp32 in place).  dbd_head_major: dbd is laid out [H][B][T][T].
    drop_p > 0 with probs_drop=None: the mask is regenerated from (drop_key, index) instead of read off probs_drop."""
    bsb, bsh = (T * T, B * T * T) if dbd_head_major else (0, 0)
    L.check(L.load().a3t_relpos_softmax_bwd(_ptr(probs), _dt(probs), _ptr(dprobs), _dt(dprobs), _ptr(ds), _ptr(dbd), _dt(dbd), B, H,
                                            T, T * T, T * T, T * T, scale, _ptr(probs_drop), drop_p, bsb, bsh, drop_key,
                                            _ptr(rowscale), _stream()), "softmax_bwd")


def attn_fused_supported(dk, T):
    """Mirror of attn_shape_ok (csrc/attn_fused.hip): shapes outside fall back to the materialised attention path."""
    return dk % 32 == 0 and dk <= 192 and dk != 160 and T % 8 == 0 and 8 <= T <= 4096


def _attn_q_operands(qu, qv, qkv, pos_bias):
    """(qu pointer, qv pointer, ldq, bias_u pointer, bias_v pointer): with pos_bias = (pos_bias_u, pos_bias_v) the kernel reads q
    itself (first d columns of qkv) and adds the biases as it loads its query fragments; qu / qv are then not needed."""
    d = qkv.shape[1] // 3
    if pos_bias is None:
        return _ptr(qu), _ptr(qv), d, None, None
    return _ptr(qkv), _ptr(qkv), 3 * d, _ptr(pos_bias[0]), _ptr(pos_bias[1])


def attn_fwd(qu, qv, qkv, P, keymask, ctx, lse, B, H, T, scale, drop=(0.0, 0), pos_bias=None):
    """Fused legacy rel-pos attention forward: ctx[b, :, h, :] = dropout(softmax(((q+u) k^T + shift((q+v) P^T)) * scale)) v.
    qu / qv / ctx [B*T][d], qkv [B*T][3d] (q | k | v), P [T][d], all bf16; lse [B][H][T] fp32.
    pos_bias=(u, v) (fp32 [d]): qu / qv may be None, q + u / q + v are formed inside the kernel."""
    d = qkv.shape[1] // 3
    dk = d // H
    kk = qkv.view(-1)[d:]
    vv = qkv.view(-1)[2 * d:]
    pqu, pqv, ldq, pbu, pbv = _attn_q_operands(qu, qv, qkv, pos_bias)
    L.check(L.load().a3t_attn_fwd(pqu, pqv, _ptr(kk), _ptr(vv), _ptr(P), _ptr(keymask), _ptr(ctx), _ptr(lse),
                                  B, H, T, dk, ldq, 3 * d, d, d, scale, drop[0], drop[1], pbu, pbv, _stream()), "attn_fwd")


def attn_fwd_train(qu, qv, qkv, P, keymask, ctx, lse, probs, probs_drop, rowscale, B, H, T, scale, drop=(0.0, 0), pos_bias=None):
    """a3t_attn_fwd for training steps: also stores un-normalised probabilities (probs, probs_drop [B][H][T][T] bf16) and
    rowscale [B][H][T] = 1 / row sum for the materialised backward.  probs_drop=None with dropout on: ONE tensor, the mask in the
    sign bits of probs (attn_bwd_ds(signed_probs=True), gemm(a_signmask=True, alpha=1/(1-p)) read it)."""
    d = qkv.shape[1] // 3
    dk = d // H
    kk = qkv.view(-1)[d:]
    vv = qkv.view(-1)[2 * d:]
    pqu, pqv, ldq, pbu, pbv = _attn_q_operands(qu, qv, qkv, pos_bias)
    e0 = None
    if PROFILE is not None:      # bench.py: the fused attention forward sits in the per-kernel table next to the GEMMs
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    L.check(L.load().a3t_attn_fwd_train(pqu, pqv, _ptr(kk), _ptr(vv), _ptr(P), _ptr(keymask), _ptr(ctx), _ptr(lse),
                                        _ptr(probs), _ptr(probs_drop), _ptr(rowscale), B, H, T, dk, ldq, 3 * d, d, d, scale,
                                        drop[0], drop[1], pbu, pbv, _stream()), "attn_fwd_train")
    if e0 is not None:
        e1.record()
        PROFILE.append((f"attn_fwd32_kernel<{dk // 32}, {'true' if drop[0] > 0 else 'false'}, true, false, false, {'true' if (drop[0] > 0 and probs_drop is None) else 'false'}>", 3 * 2.0 * B * H * T * T * dk, e0, e1,
                        (T, T, dk, B * H, 1, 1)))


def attn_fwd_plain(qkv, keymask, ctx, lse, B, H, T, scale, drop=(0.0, 0)):
    """attn_fwd without the positional term: ctx[b, :, h, :] = dropout(softmax(q k^T * scale)) v, q | k | v the thirds of qkv
    [B*T][3d] (bf16); the band-free instantiation of the fused kernels."""
    d = qkv.shape[1] // 3
    if qkv.dtype != torch.bfloat16 or ctx.dtype != torch.bfloat16 or qkv.shape[0] < B * T or ctx.numel() < B * T * d or \
            lse.numel() < B * H * T or keymask.numel() < B * T or d % H:
        raise ValueError("attn_fwd_plain: shapes do not fit")
    L.check(L.load().a3t_attn_fwd_plain(_ptr(qkv), _ptr(qkv.view(-1)[d:]), _ptr(qkv.view(-1)[2 * d:]), _ptr(keymask), _ptr(ctx),
                                        _ptr(lse), B, H, T, d // H, 3 * d, 3 * d, d, scale, drop[0], drop[1], _stream()),
            "attn_fwd_plain")


def attn_fwd_train_plain(qkv, keymask, ctx, lse, probs, probs_drop, rowscale, B, H, T, scale, drop=(0.0, 0)):
    """attn_fwd_train without the positional term; probs / probs_drop / rowscale as there (probs_drop=None with dropout on: the
    mask in the sign bits of probs)."""
    d = qkv.shape[1] // 3
    n = B * H * T * T
    if qkv.dtype != torch.bfloat16 or ctx.dtype != torch.bfloat16 or probs.dtype != torch.bfloat16 or qkv.shape[0] < B * T or \
            ctx.numel() < B * T * d or lse.numel() < B * H * T or rowscale.numel() < B * H * T or keymask.numel() < B * T or \
            probs.numel() < n or (probs_drop is not None and (probs_drop.numel() < n or probs_drop.dtype != torch.bfloat16)) or d % H:
        raise ValueError("attn_fwd_train_plain: shapes do not fit")
    L.check(L.load().a3t_attn_fwd_train_plain(_ptr(qkv), _ptr(qkv.view(-1)[d:]), _ptr(qkv.view(-1)[2 * d:]), _ptr(keymask),
                                              _ptr(ctx), _ptr(lse), _ptr(probs), _ptr(probs_drop), _ptr(rowscale), B, H, T, d // H,
                                              3 * d, 3 * d, d, scale, drop[0], drop[1], _stream()), "attn_fwd_train_plain")


def attn_scale_rows(x, rowscale, y, B, H, T):
    d = x.shape[1]
    L.check(L.load().a3t_attn_scale_rows(_ptr(x), _ptr(rowscale), _ptr(y), B, H, T, d // H, _stream()), "attn_scale_rows")


def attn_bwd_ds(dctx, ctx, qkv, probs, rowscale, ds, dbd, B, H, T, scale, drop=(0.0, 0), dbd_head_major=False, signed_probs=False,
                ds_bs=0):
    """dS and the compact dBD from the saved un-normalised probabilities of attn_fwd_train (dP = dctx V^T is never stored; the row
    term delta = dctx . ctx is formed in the kernel): replaces the dprobs GEMM + relpos_softmax_bwd.  qkv: [B*T, 3d], V in
    columns 2d..3d; ctx: the forward's output [B*T, d].  signed_probs: probs is the sign-tagged single tensor of
    attn_fwd_train(probs_drop=None) -- the dropout mask is read off its sign bits.  dbd=None: only dS is written, into (b, h) blocks
    ds_bs elements apart (T zeros in front of each): the compact dBD matrix is then the view ds.view(-1)[-(T-1):] with row stride T + 1."""
    d = dctx.shape[1]
    v = qkv.view(-1)[2 * d:]
    bsb, bsh = ((T * T, B * T * T) if dbd_head_major else (0, 0))
    L.check(L.load().a3t_attn_bwd_ds(_ptr(dctx), _ptr(ctx), _ptr(v), _ptr(probs), _ptr(rowscale), _ptr(ds), _ptr(dbd), B, H, T,
                                     d // H, d, 3 * d, bsb, bsh, scale, drop[0], drop[1], 1 if signed_probs else 0, ds_bs, _stream()), "attn_bwd_ds")


def attn_bwd_dpos_plan(B, H, T, dk):
    """(rows per tile, row tiles, batch elements per workgroup, grid) of attn_bwd_dpos, or None where it does not take the problem
    (host only: csrc/attn_dpos.hip, dpos_plan)."""
    out = (ctypes.c_int * 4)()
    if not L.load().a3t_attn_bwd_dpos_plan(int(B), int(H), int(T), int(dk), out):
        return None
    return tuple(out)


def attn_bwd_dpos_ws(B, H, T, dk):
    """fp32 workspace elements of attn_bwd_dpos (0 where the path does not take the problem)."""
    return int(L.load().a3t_attn_bwd_dpos_ws(int(B), int(H), int(T), int(dk)))


def attn_bwd_dpos(dbd, qv, ws, dP16, B, H, T, dbd_rs, dbd_bs, dP=None):
    """dP16[r, h*dk + n] = bf16(sum_b sum_i dbd[b, h][i, r] qv[b*T + i, h*dk + n]): the gradient of linear_pos' output as a streaming
    product over groups of batch elements + a fold in fixed order (no atomics).  dbd: the compact matrix (dbd_rs = T) or its view of dS
    (dbd_rs = T + 1), (b, h) blocks dbd_bs = (per b, per h) elements apart; ws: attn_bwd_dpos_ws floats; dP: optional fp32 copy."""
    d = qv.shape[1]
    L.check(L.load().a3t_attn_bwd_dpos(_ptr(dbd), _ptr(qv), _ptr(ws), _ptr(dP16), _ptr(dP), B, H, T, d // H, int(dbd_rs),
                                       int(dbd_bs[0]), int(dbd_bs[1]), _stream()), "attn_bwd_dpos")


def mask_fill(speech, masked, mask_feature, out):
    M, C = out.shape
    L.check(L.load().a3t_mask_fill(_ptr(speech), _ptr(masked), _ptr(mask_feature), _ptr(out), _dt(out), M, C,
                                   _stream()), "mask_fill")


def embed_finish_fwd(e, emb, seg, text, spos, tpos, xs, B, Tm, Tp, D, xscale, drop=(0.0, 0), spk=None):
    L.check(L.load().a3t_embed_finish_fwd(_ptr(e), _ptr(emb), _ptr(seg), _ptr(text), _ptr(spos), _ptr(tpos), _ptr(xs),
                                          B, Tm, Tp, D, xscale, drop[0], drop[1], _ptr(spk), _stream()), "embed_fwd")


def embed_finish_bwd(dxs, e, text, spos, tpos, de, demb, dseg, B, Tm, Tp, D, V, nseg, xscale, drop=(0.0, 0)):
    L.check(L.load().a3t_embed_finish_bwd(_ptr(dxs), _ptr(e), _ptr(text), _ptr(spos), _ptr(tpos), _ptr(de),
                                          _ptr(demb), _ptr(dseg), B, Tm, Tp, D, V, nseg, xscale, drop[0], drop[1],
                                          _stream()), "embed_bwd")


def _f32c(t, n, what):
    """t is a contiguous fp32 tensor of at least n elements (what the absolute-position kernels index without a stride)."""
    if t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
        raise ValueError(f"{what}: expected a contiguous float32 tensor of >= {n} elements")
    return t


def embed_finish_abs_fwd(e, emb, seg, text, spos, tpos, pe, alpha, xs, B, Tm, Tp, D, xscale, drop=(0.0, 0), spk=None):
    """embed_finish_fwd with absolute positions: relu(e) * xscale + pe[t] | emb[text] * xscale + pe[t - Tm], or with
    alpha = (alpha_s, alpha_t) (device scalars) relu(e) + alpha_s * pe[t] | emb[text] + alpha_t * pe[t - Tm]; then dropout, + seg,
    + spk.  pe: [>= max(Tm, Tp)][D] fp32, row t = PE(t)."""
    _f32c(pe, max(Tm, Tp) * D, "pe")
    _f32c(xs, B * (Tm + Tp) * D, "xs")
    if Tm:
        _f32c(e, B * Tm * D, "e")
    if Tp and (text.dtype != torch.int64 or text.numel() < B * Tp):
        raise ValueError("text: expected int64 [B][Tp]")
    if seg is not None and (spos.numel() < B * Tm or tpos.numel() < B * Tp or spos.dtype != torch.int64 or tpos.dtype != torch.int64):
        raise ValueError("spos / tpos: expected int64 [B][Tm] / [B][Tp]")
    a_s, a_t = alpha if alpha is not None else (None, None)
    L.check(L.load().a3t_embed_finish_abs_fwd(_ptr(e), _ptr(emb), _ptr(seg), _ptr(text), _ptr(spos), _ptr(tpos), _ptr(pe),
                                              _ptr(a_s), _ptr(a_t), _ptr(xs), B, Tm, Tp, D, xscale, drop[0], drop[1], _ptr(spk),
                                              _stream()), "embed_abs_fwd")


def embed_finish_abs_partials(B, Tm, Tp, D):
    """Floats of scratch embed_finish_abs_bwd needs for the per-workgroup partial sums of the alpha gradients."""
    return int(L.load().a3t_embed_finish_abs_partials(B, Tm, Tp, D))


def embed_finish_abs_bwd(dxs, e, text, spos, tpos, pe, de, demb, dseg, dalpha, partial, B, Tm, Tp, D, V, nseg, xscale,
                         drop=(0.0, 0)):
    """Backward of embed_finish_abs_fwd.  dalpha = (dalpha_s, dalpha_t) (accumulated into; partial = fp32 scratch of
    embed_finish_abs_partials floats) or None for the plain encoding."""
    _f32c(pe, max(Tm, Tp) * D, "pe")
    _f32c(dxs, B * (Tm + Tp) * D, "dxs")
    if Tm:
        _f32c(e, B * Tm * D, "e")
        _f32c(de, B * Tm * D, "de")
    if Tp:
        _f32c(demb, V * D, "demb")
    d_s, d_t = dalpha if dalpha is not None else (None, None)
    if dalpha is not None:
        _f32c(partial, embed_finish_abs_partials(B, Tm, Tp, D), "partial")
    L.check(L.load().a3t_embed_finish_abs_bwd(_ptr(dxs), _ptr(e), _ptr(text), _ptr(spos), _ptr(tpos), _ptr(pe), _ptr(de),
                                              _ptr(demb), _ptr(dseg), _ptr(d_s), _ptr(d_t), _ptr(partial), B, Tm, Tp, D, V, nseg,
                                              xscale, drop[0], drop[1], _stream()), "embed_abs_bwd")


def scale_add_pos(x, pe, y, B, T, D, s, drop=(0.0, 0)):
    """y[b][t] = dropout(x[b][t] * s + pe[t]): the decoder entry of a transformer model."""
    _f32c(x, B * T * D, "x")
    _f32c(y, B * T * D, "y")
    _f32c(pe, T * D, "pe")
    L.check(L.load().a3t_scale_add_pos(_ptr(x), _ptr(pe), _ptr(y), B, T, D, s, drop[0], drop[1], _stream()), "scale_add_pos")


def softmax_plain_fwd(ac, keymask, probs, B, H, T, scale, probs_drop=None, drop=(0.0, 0)):
    """relpos_softmax_fwd without the positional term: probs = softmax_j(ac * scale) under the key mask."""
    n = B * H * T * T
    if ac.numel() < n or probs.numel() < n or keymask.numel() < B * T or (probs_drop is not None and probs_drop.numel() < n):
        raise ValueError("softmax_plain_fwd: shapes do not fit")
    L.check(L.load().a3t_softmax_plain_fwd(_ptr(ac), _dt(ac), _ptr(keymask), _ptr(probs), _dt(probs), B, H, T, T * T, T * T, scale,
                                           _ptr(probs_drop), drop[0], drop[1], _stream()), "softmax_plain_fwd")


def softmax_plain_bwd(probs, dprobs, ds, B, H, T, scale, probs_drop=None, drop_p=0.0, drop_key=0, rowscale=None):
    """relpos_softmax_bwd without dbd: ds = probs * (dprobs - sum_j dprobs * probs) * scale (ds may be dprobs itself in fp32)."""
    n = B * H * T * T
    if probs.numel() < n or dprobs.numel() < n or ds.numel() < n or (probs_drop is not None and probs_drop.numel() < n) or \
            (rowscale is not None and rowscale.numel() < B * H * T):
        raise ValueError("softmax_plain_bwd: shapes do not fit")
    L.check(L.load().a3t_softmax_plain_bwd(_ptr(probs), _dt(probs), _ptr(dprobs), _dt(dprobs), _ptr(ds), _dt(ds), B, H, T, T * T,
                                           T * T, T * T, scale, _ptr(probs_drop), drop_p, drop_key, _ptr(rowscale), _stream()),
            "softmax_plain_bwd")


def scale(x, y, s):
    L.check(L.load().a3t_scale(_ptr(x), _ptr(y), x.numel(), s, _stream()), "scale")


def scale_dev(x, y, s):
    L.check(L.load().a3t_scale_dev(_ptr(x), _ptr(y), x.numel(), _ptr(s), _stream()), "scale_dev")


def axpy(x, y, a=1.0):
    L.check(L.load().a3t_axpy(_ptr(x), _ptr(y), x.numel(), a, _stream()), "axpy")


def attn_bias_fold(slots, S, d, gu, gv, gbqkv):
    L.check(L.load().a3t_attn_bias_fold(_ptr(slots), S, d, _ptr(gu), _ptr(gv), _ptr(gbqkv), _stream()), "attn_bias_fold")


def cast_bf16(x, y):
    L.check(L.load().a3t_cast_bf16(_ptr(x), _ptr(y), x.numel(), _stream()), "cast_bf16")


def cast_bf16_conv_t(src_flat, dst, src_off, dst_off, N, taps, C):
    """Transposed, tap-reversed bf16 shadows of src_off.numel() conv weights [N][taps][C] of the flat fp32 buffer."""
    L.check(L.load().a3t_cast_bf16_conv_t(_ptr(src_flat), _ptr(dst), _ptr(src_off), _ptr(dst_off), src_off.numel(), N, taps, C,
                                          _stream()), "cast_bf16_conv_t")


def split_bf16(x, hi, lo):
    L.check(L.load().a3t_split_bf16(_ptr(x), _ptr(hi), _ptr(lo), x.numel(), _stream()), "split_bf16")


def slice_rows(x, y, B, T, Tm, D, reverse_add=False):
    L.check(L.load().a3t_slice_rows(_ptr(x), _ptr(y), _dt(y), B, T, Tm, D, int(reverse_add), _stream()), "slice_rows")


def concat_rows(speech, text, xs, B, Tm, Tp, D):
    """xs[B][Tm+Tp][D] = speech[B][Tm][D] | text[B][Tp][D] along time (fp32)."""
    L.check(L.load().a3t_concat_rows(_ptr(speech), _ptr(text), _ptr(xs), B, Tm, Tp, D, _stream()), "concat_rows")


def concat_rows_ragged(speech, text, xs, slens, tlens, B, Tm, Tp, D, speech_bs=None, text_bs=None):
    """xs[B][Tm+Tp][D]: row b = speech[b][:slens[b]] | text[b][:tlens[b]] | zeros (fp32; slens / tlens device int32 [B]).
    speech_bs / text_bs: elements between the sources' batch rows (default Tm * D / Tp * D); 0 = one source for every row."""
    L.check(L.load().a3t_concat_rows_ragged(_ptr(speech), _ptr(text), _ptr(xs), _ptr(_i32(slens, "slens")),
                                            _ptr(_i32(tlens, "tlens")), B, Tm, Tp, D, Tm * D if speech_bs is None else speech_bs,
                                            Tp * D if text_bs is None else text_bs, _stream()), "concat_rows_ragged")


def split_rows(dxs, dspeech, dtext, B, Tm, Tp, D):
    """The backward of concat_rows: dspeech / dtext = the two parts of dxs (stored)."""
    L.check(L.load().a3t_split_rows(_ptr(dxs), _ptr(dspeech), _ptr(dtext), B, Tm, Tp, D, _stream()), "split_rows")


def reflect_pad(x, out, pad):
    B, N = x.shape
    L.check(L.load().a3t_reflect_pad(_ptr(x), _ptr(out), B, N, pad, out.shape[1], _stream()), "reflect_pad")


def reflect_pad_ragged(x, out, pad, lens, host_lens):
    """reflect_pad with each row reflected about its own ends (a3t_reflect_pad_ragged): lens = device int32 [B], host_lens
    = the same lengths on the host, checked here -- torch.stft refuses a row that is not longer than the pad, and so does this."""
    B, N = x.shape
    host_lens = [int(n) for n in host_lens]
    if len(host_lens) != B or lens.numel() != B:
        raise ValueError(f"reflect_pad_ragged: {B} rows, {len(host_lens)} host lengths, {lens.numel()} device lengths")
    for b, n in enumerate(host_lens):
        if n <= pad or n > N:
            raise ValueError(f"reflect_pad_ragged: row {b} has {n} samples; reflection by {pad} needs {pad} < n <= {N}")
    L.check(L.load().a3t_reflect_pad_ragged(_ptr(x), _ptr(out), _ptr(_i32(lens, "lens")), B, N, pad, out.shape[1], _stream()),
            "reflect_pad_ragged")


def stft_amp(S, amp, nbins):
    L.check(L.load().a3t_stft_amp(_ptr(S), _ptr(amp), amp.shape[0], nbins, amp.shape[1], _stream()), "stft_amp")


def logmel_finish(mel, olens, B, F, C):
    L.check(L.load().a3t_logmel_finish(_ptr(mel), _ptr(olens), B, F, C, _stream()), "logmel_finish")


def mlm_loss(before, after, target, masked, loss_out, d_before, d_after, scratch, l2=False, gscale=1.0):
    M, C = before.shape
    L.check(L.load().a3t_mlm_loss(_ptr(before), _ptr(after), _ptr(target), _ptr(masked), _ptr(loss_out),
                                  _ptr(d_before), _ptr(d_after), _ptr(scratch), M, C, int(l2), gscale, _stream()),
            "mlm_loss")


def loss_scratch_floats(M):
    return L.load().a3t_mlm_loss_scratch_floats(M)


def sumsq(g, partial):
    L.check(L.load().a3t_sumsq(_ptr(g), g.numel(), _ptr(partial), _stream()), "sumsq")


def clip_adam(p, g, m, v, partial, norm_out, lr, step, clip=1.0, gscale=1.0, betas=(0.9, 0.999), eps=1e-8):
    L.check(L.load().a3t_clip_adam(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(partial), _ptr(norm_out), p.numel(), lr,
                                   betas[0], betas[1], eps, step, clip, gscale, _stream()), "clip_adam")


def clip_adam_noam(p, g, m, v, partial, norm_out, state, base_lr, model_size, warmup, clip=1.0, gscale=1.0,
                   betas=(0.9, 0.999), eps=1e-8):
    """clip + Adam + NoamLR with the step counter on the device (state int32[2]: applied, skipped)."""
    L.check(L.load().a3t_clip_adam_noam(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(partial), _ptr(norm_out), p.numel(),
                                        _ptr(state), base_lr, float(model_size), float(warmup), betas[0], betas[1], eps,
                                        clip, gscale, _stream()), "clip_adam_noam")


def sgd_step(p, g, lr, gscale=1.0):
    """p -= (lr * gscale) * g on the flat fp32 buffers, one launch: torch.optim.SGD(lr) without momentum, weight decay, clipping
    or a finite-gradient guard (a3t_sgd_step; the step is rounded to fp32 once, the product and the difference separately)."""
    if p.dtype != torch.float32 or g.dtype != torch.float32 or p.numel() != g.numel() or not (p.is_contiguous() and g.is_contiguous()):
        raise ValueError("sgd_step: p and g must be contiguous fp32 buffers of one size")
    L.check(L.load().a3t_sgd_step(_ptr(p), _ptr(g), p.numel(), float(lr), float(gscale), _stream()), "sgd_step")


def pwg_gate(y, c, out):
    T, H = out.shape
    L.check(L.load().a3t_pwg_gate(_ptr(y), _ptr(c), _ptr(out), T, H, _stream()), "pwg_gate")


def pwg_res_skip(o, x, skips):
    T, R = x.shape
    L.check(L.load().a3t_pwg_res_skip(_ptr(o), _ptr(x), _ptr(skips), T, R, skips.shape[1], _stream()), "pwg_res_skip")


def _i32(t, what):
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int32 tensor")
    return t


def _rows_lens(what, x, lens):
    """B, T, C of x [T][C] or [B][T][C]; lens (None or device int32 [B]) checked against B."""
    B = x.shape[0] if x.dim() == 3 else 1
    if lens is not None and _i32(lens, "lens").numel() != B:
        raise ValueError(f"{what}: {lens.numel()} lengths for {B} rows")
    return (B, *x.shape[-2:])


def pwg_upsample(c, w, out, scale_, lens=None, mul=1):
    """c [Tin][C] or [B][Tin][C] (contiguous) -> out [.., Tin*scale, C].  lens (device int32 [B]): row b is valid for
    lens[b] * mul input rows and zero behind."""
    B, Tin, C = _rows_lens("pwg_upsample", c, lens)
    if lens is None:
        rc = L.load().a3t_pwg_upsample(_ptr(c), _ptr(w), _ptr(out), B, Tin, C, scale_, _stream())
    else:
        rc = L.load().a3t_pwg_upsample_ragged(_ptr(c), _ptr(w), _ptr(out), _ptr(lens), mul, B, Tin, C, scale_, _stream())
    L.check(rc, "pwg_upsample")


def replicate_pad(x, y, pad, lens=None):
    """x [T][C] or [B][T][C] (contiguous) -> y [.., T + 2 pad, C].  lens (device int32 [B]): row b is clamped to its own
    [0, lens[b] - 1]."""
    B, T, C = _rows_lens("replicate_pad", x, lens)
    if lens is None:
        rc = L.load().a3t_replicate_pad(_ptr(x), _ptr(y), B, T, C, pad, _stream())
    else:
        rc = L.load().a3t_replicate_pad_ragged(_ptr(x), _ptr(y), _ptr(lens), B, T, C, pad, _stream())
    L.check(rc, "replicate_pad")


def zero_tail(x, lens, mul, B, T):
    """x [B*T][C] (or [B][T][C]): rows t >= lens[b] * mul of every b are set to 0."""
    C = x.shape[-1]
    L.check(L.load().a3t_zero_tail(_ptr(x), _ptr(_i32(lens, "lens")), mul, B, T, C, _stream()), "zero_tail")


def _ragged_f32(what, *ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError(f"{what}: tensors must be contiguous fp32")


def layernorm_fwd_ragged(x, g, b, y, mean, rstd, lens, B, T, eps):
    """layernorm_fwd over x [B*T][D] whose rows t >= lens[b] are stored as 0; mean / rstd: both or None."""
    M, D = x.shape
    _ragged_f32("layernorm_fwd_ragged", x, y, mean, rstd)
    if M != B * T or y.shape != x.shape or lens.numel() != B:
        raise ValueError("layernorm_fwd_ragged: shapes do not fit")
    L.check(L.load().a3t_layernorm_fwd_ragged(_ptr(x), _ptr(g), _ptr(b), _ptr(y), _ptr(mean), _ptr(rstd),
                                              _ptr(_i32(lens, "lens")), B, T, D, eps, _stream()), "ln_fwd_ragged")


def glu_dwconv_fwd_ragged(g, wdw, bdw, glu, z, lens, B, Tseq):
    """glu_dwconv_fwd whose taps read 0 behind lens[b]; glu and z are 0 there."""
    M, C = glu.shape
    _ragged_f32("glu_dwconv_fwd_ragged", g, glu, z)
    if M != B * Tseq or g.shape != (M, 2 * C) or z.shape != glu.shape or lens.numel() != B:
        raise ValueError("glu_dwconv_fwd_ragged: shapes do not fit")
    L.check(L.load().a3t_glu_dwconv_fwd_ragged(_ptr(g), _ptr(wdw), _ptr(bdw), _ptr(glu), _ptr(z), _ptr(_i32(lens, "lens")),
                                               B, Tseq, C, wdw.shape[1], _stream()), "glu_dwconv_fwd_ragged")


def relpos_softmax_fwd_ragged(ac, bd, lens, probs, B, H, T, scale):
    """relpos_softmax_fwd with per-row lengths: key mask j < lens[b], rel_shift at lens[b], query rows behind it 0.  The
    library refuses anything but fp32 scores and probabilities."""
    if min(ac.numel(), bd.numel(), probs.numel()) < B * H * T * T or lens.numel() != B:
        raise ValueError("relpos_softmax_fwd_ragged: shapes do not fit")
    L.check(L.load().a3t_relpos_softmax_fwd_ragged(_ptr(ac), _ptr(bd), _dt(ac), _ptr(_i32(lens, "lens")), _ptr(probs),
                                                   _dt(probs), B, H, T, T * T, T * T, T * T, scale, _stream()),
            "softmax_fwd_ragged")


def _tile_list(what, tiles, B, Tw):
    """(pointer, ntiles) of an optional tile list (vocoder.pwg_tile_list) for B rows of Tw samples (the contract of
    csrc/wave_tiles.h: what can be checked on the host is, the kernels trust the entries); ntiles < 0: nothing to do."""
    if tiles is None:
        return None, 0
    if tiles.dim() != 2 or tiles.shape[1] != 4:
        raise ValueError(f"{what}: tiles must be (ntiles, 4), got {tuple(tiles.shape)}")
    if tiles.shape[0] > B * ((Tw + 255) // 256):
        raise ValueError(f"{what}: {tiles.shape[0]} tiles do not fit {B} rows of {Tw} samples")
    _i32(tiles, "tiles")
    if tiles.shape[0] == 0:      # (an empty tensor has no address: NULL would mean "dense")
        return None, -1
    return _ptr(tiles), tiles.shape[0]


def pwg_block(x, cu, wt0, b0, wt1, b1, g, skips, B, Tw, dil, tiles=None):
    """Fused residual block, x and skips updated in place.  tiles None: all rows Tw samples long (a3t_pwg_block); else rows of
    different length (a3t_pwg_block_ragged), tiles: device int32 [ntiles][4] = {row b, first sample t0, valid samples W_b, 0}
    (vocoder.pwg_tile_list).  The kernel indexes x / cu / g / skips with the list's entries unchecked: 0 <= b < B, t0 < W_b <= Tw
    are the caller's to guarantee."""
    for name, t, C in (("x", x, 64), ("cu", cu, 80), ("g", g, 64), ("skips", skips, 64)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != B * Tw * C:
            raise ValueError(f"pwg_block: {name} must be a contiguous fp32 [{B * Tw}][{C}] tensor")
    args = (_ptr(x), _ptr(cu), _ptr(wt0), _ptr(b0), _ptr(wt1), _ptr(b1), _ptr(g), _ptr(skips))
    tp, nt = _tile_list("pwg_block", tiles, B, Tw)
    if tiles is None:
        L.check(L.load().a3t_pwg_block(*args, B, Tw, dil, _stream()), "pwg_block")
    elif nt > 0:
        L.check(L.load().a3t_pwg_block_ragged(*args, tp, nt, B, Tw, dil, _stream()), "pwg_block")


def cast_f16_sat(src, dst):
    """dst (fp16) = src (fp32) rounded to nearest even and saturated to +-65504 (a3t_cast_f16_sat)."""
    if src.dtype != torch.float32 or dst.dtype != torch.float16 or src.numel() != dst.numel() \
            or not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("cast_f16_sat: src must be contiguous fp32, dst contiguous fp16 of the same size")
    L.check(L.load().a3t_cast_f16_sat(_ptr(src), _ptr(dst), src.numel(), _stream()), "cast_f16_sat")


def pwg_block_f16(x_in, x_out, cu16, w0h, b0, w1h, b1, skips, tiles, B, Tw, dil):
    """Fused residual block in one launch on the 16-bit MFMA (a3t_pwg_block_f16): x_in -> x_out (two different buffers), skips in
    place.  cu16 / w0h / w1h fp16 (cast_f16_sat, vocoder.pack_pwg_block_f16); tiles: None = all rows Tw samples long, else the
    list of pwg_block."""
    for name, t, C, dt in (("x_in", x_in, 64, torch.float32), ("x_out", x_out, 64, torch.float32), ("cu16", cu16, 80, torch.float16),
                           ("skips", skips, 64, torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != B * Tw * C:
            raise ValueError(f"pwg_block_f16: {name} must be a contiguous {dt} [{B * Tw}][{C}] tensor")
    for name, t, shape, dt in (("w0h", w0h, (272, 128), torch.float16), ("w1h", w1h, (64, 128), torch.float16),
                               ("b0", b0, (128,), torch.float32), ("b1", b1, (128,), torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"pwg_block_f16: {name} must be a contiguous {dt} tensor of shape {shape}")
    tp, nt = _tile_list("pwg_block_f16", tiles, B, Tw)
    if nt < 0:
        return
    L.check(L.load().a3t_pwg_block_f16(_ptr(x_in), _ptr(x_out), _ptr(cu16), _ptr(w0h), _ptr(b0), _ptr(w1h), _ptr(b1),
                                       _ptr(skips), tp, nt, B, Tw, dil, _stream()), "pwg_block_f16")


def leaky_relu(x, y, slope):
    """y = x > 0 ? x : x * slope (a3t_leaky_relu), contiguous fp32 of the same size; y may be x."""
    _ragged_f32("leaky_relu", x, y)
    if x.numel() != y.numel():
        raise ValueError("leaky_relu: x and y must have the same size")
    L.check(L.load().a3t_leaky_relu(_ptr(x), _ptr(y), x.numel(), slope, _stream()), "leaky_relu")


def _hfg_conv_args(what, x, bias, R, y, acc, B, Tw, tiles):
    """What hfg_conv and hfg_conv_f16 check alike: x / R / y / acc fp32 [B*Tw][C], x overlapping neither y nor acc, y not acc, a
    bias of C entries -> (C, tile pointer, ntiles) as _tile_list."""
    C = x.shape[-1]
    for name, t in (("x", x), ("R", R), ("y", y), ("acc", acc)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape[-1] != C or t.numel() != B * Tw * C):
            raise ValueError(f"{what}: {name} must be a contiguous fp32 [{B * Tw}][{C}] tensor")
    nbytes = 4 * B * Tw * C
    for name, t in (("y", y), ("acc", acc)):      # other tiles read x[t +- halo]: no output may overlap the input, or the other
        for oname, o in (("x", x), ("acc", acc if name == "y" else None)):
            if t is not None and o is not None and abs(t.data_ptr() - o.data_ptr()) < nbytes:
                raise ValueError(f"{what}: {name} overlaps {oname}")
    _ragged_f32(what, bias)
    if bias is not None and bias.numel() != C:
        raise ValueError(f"{what}: bias must have {C} entries")
    return (C,) + _tile_list(what, tiles, B, Tw)


def hfg_conv(x, wt, bias, y, B, Tw, dil, slope, R=None, acc=None, alpha=1.0, acc_add=False, tiles=None):
    """One HiFi-GAN residual-unit convolution (a3t_hfg_conv): v = bias + conv(leaky(x, slope)) (+ R); y = v (y may be None) and
    acc = alpha * v or, with acc_add, acc += alpha * v (acc may be None).  x / R / y / acc fp32 [B*Tw][C], C in {32, 64};
    wt [taps*C][C] k-major (vocoder.pack_hifigan_conv), taps odd <= 11.  R may be y; x must overlap neither y nor acc (checked here).
    tiles: as pwg_block, the kernel trusts the list's entries."""
    C = x.shape[-1]
    if wt.dim() != 2 or wt.shape[1] != C or wt.shape[0] % C:
        raise ValueError(f"hfg_conv: wt must be [taps*{C}][{C}], got {tuple(wt.shape)}")
    C, tp, nt = _hfg_conv_args("hfg_conv", x, bias, R, y, acc, B, Tw, tiles)
    _ragged_f32("hfg_conv", wt)
    if nt < 0:
        return
    L.check(L.load().a3t_hfg_conv(_ptr(x), _ptr(wt), _ptr(bias), _ptr(R), _ptr(y), _ptr(acc), alpha, int(bool(acc_add)), slope,
                                  tp, nt, B, Tw, C, wt.shape[0] // C, dil, _stream()), "hfg_conv")


def hfg_conv_f16(x, wf, bias, y, B, Tw, dil, slope, R=None, acc=None, alpha=1.0, acc_add=False, tiles=None):
    """hfg_conv with fp16 operands on the 16-bit MFMA (a3t_hfg_conv_f16): leaky(x) is rounded to fp16 (saturated) on its way into
    the product, wf holds the fp16 weight fragments [taps*C/16][C/32][64][8] of vocoder.pack_hifigan_conv_f16; C in {32, 64, 128,
    256}.  Everything else, fp32 accumulation included, as hfg_conv."""
    C = x.shape[-1]
    if wf.dtype != torch.float16 or not wf.is_contiguous() or wf.dim() != 4 or C % 32 or tuple(wf.shape[1:]) != (C // 32, 64, 8) \
            or wf.shape[0] % (C // 16):
        raise ValueError(f"hfg_conv_f16: wf must be a contiguous fp16 [taps*{C // 16}][{C // 32}][64][8] tensor, got "
                         f"{wf.dtype} {tuple(wf.shape)}")
    C, tp, nt = _hfg_conv_args("hfg_conv_f16", x, bias, R, y, acc, B, Tw, tiles)
    if nt < 0:
        return
    L.check(L.load().a3t_hfg_conv_f16(_ptr(x), _ptr(wf), _ptr(bias), _ptr(R), _ptr(y), _ptr(acc), alpha, int(bool(acc_add)), slope,
                                      tp, nt, B, Tw, C, wf.shape[0] // (C // 16), dil, _stream()), "hfg_conv_f16")


def hfg_out(x, w, bias, y, B, Tw, slope, tiles=None):
    """y [B*Tw] = tanh(bias + conv_K(leaky(x, slope))) (a3t_hfg_out): x fp32 [B*Tw][C], w [K][C] (tap, in channel), bias [1] or
    None.  tiles: as hfg_conv."""
    C = x.shape[-1]
    _ragged_f32("hfg_out", x, w, bias, y)
    if w.dim() != 2 or w.shape[1] != C or x.numel() != B * Tw * C or y.numel() != B * Tw:
        raise ValueError("hfg_out: shapes do not fit")
    tp, nt = _tile_list("hfg_out", tiles, B, Tw)
    if nt < 0:
        return
    L.check(L.load().a3t_hfg_out(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), slope, tp, nt, B, Tw, C, w.shape[0], _stream()), "hfg_out")


def _tile_wmin(tiles, wmin, Tw):
    """The smallest W_b of a tile list for the kernels that reflect at a row's end: the caller's statement (host integers it
    built the list from), else read back from the list (a device synchronisation: tests and one-off calls)."""
    if tiles is None:
        return Tw
    if wmin is not None:
        return int(wmin)
    return int(tiles[:, 2].min().item()) if tiles.shape[0] else Tw


def mgan_stack(x, w, bias, y, B, Tw, dil, slope, tiles=None, wmin=None):
    """One MelGAN ResidualStack in one launch (a3t_mgan_stack): y = (bs + b2) + Ws x + W2 leaky(b1 + conv3_dil(leaky(reflect(x)))).
    x / y fp32 [B*Tw][C], C in {48, 96, 192}; w / bias from vocoder.pack_melgan_stack.  y must not overlap x.  tiles: as hfg_conv;
    wmin: the smallest W_b of the list (None: read from the list, which synchronises)."""
    C = x.shape[-1]
    Cp = (C + 31) // 32 * 32
    for name, t in (("x", x), ("y", y)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[-1] != C or t.numel() != B * Tw * C:
            raise ValueError(f"mgan_stack: {name} must be a contiguous fp32 [{B * Tw}][{C}] tensor")
    if abs(x.data_ptr() - y.data_ptr()) < 4 * B * Tw * C:
        raise ValueError("mgan_stack: y overlaps x")
    _ragged_f32("mgan_stack", w, bias)
    if tuple(w.shape) != (4 * C + Cp, Cp) or tuple(bias.shape) != (2, Cp):
        raise ValueError(f"mgan_stack: w must be [{4 * C + Cp}][{Cp}] and bias [2][{Cp}], got {tuple(w.shape)} and {tuple(bias.shape)}")
    tp, nt = _tile_list("mgan_stack", tiles, B, Tw)
    if nt < 0:
        return
    L.check(L.load().a3t_mgan_stack(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), slope, tp, nt, _tile_wmin(tiles, wmin, Tw), B, Tw, C,
                                    dil, _stream()), "mgan_stack")


def mgan_out(x, w, bias, y, B, Tw, slope, tanh=True, tiles=None, wmin=None):
    """y [B*Tw][O] = act(bias + conv_K(leaky(x, slope))) with reflection at each row's ends (a3t_mgan_out): x fp32 [B*Tw][C],
    w [O][K][C] (out channel, tap, in channel), bias [O] or None, act = tanh or identity.  tiles / wmin: as mgan_stack."""
    C = x.shape[-1]
    _ragged_f32("mgan_out", x, w, bias, y)
    if w.dim() != 3 or w.shape[2] != C or x.numel() != B * Tw * C or y.numel() != B * Tw * w.shape[0] \
            or (bias is not None and bias.numel() != w.shape[0]):
        raise ValueError("mgan_out: shapes do not fit")
    tp, nt = _tile_list("mgan_out", tiles, B, Tw)
    if nt < 0:
        return
    L.check(L.load().a3t_mgan_out(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), slope, int(bool(tanh)), tp, nt,
                                  _tile_wmin(tiles, wmin, Tw), B, Tw, C, w.shape[0], w.shape[1], _stream()), "mgan_out")


def pqmf_synthesis(x, h, y, B, Ts, tiles=None):
    """PQMF synthesis (a3t_pqmf_synthesis): x fp32 [B*Ts][S] sub-band samples, h [S][taps + 1] synthesis filters -> y [B*Ts*S].
    tiles: a list at the OUTPUT rate (Tw = Ts * S), as hfg_conv."""
    _ragged_f32("pqmf_synthesis", x, h, y)
    if h.dim() != 2 or x.shape[-1] != h.shape[0] or x.numel() != B * Ts * h.shape[0] or y.numel() != x.numel():
        raise ValueError("pqmf_synthesis: shapes do not fit")
    tp, nt = _tile_list("pqmf_synthesis", tiles, B, Ts * h.shape[0])
    if nt < 0:
        return
    L.check(L.load().a3t_pqmf_synthesis(_ptr(x), _ptr(h), _ptr(y), tp, nt, B, Ts, h.shape[0], h.shape[1] - 1, _stream()),
            "pqmf_synthesis")


SMG_PLAIN, SMG_TADE, SMG_GATE = 0, 1, 2


def smg_conv(x, wt, bias, y, B, Tw, dil=1, up=1, mode=SMG_PLAIN, m=None, stats=None, ux=1, R=None, ur=1, sigmoid=False,
             tiles=None):
    """One convolution of a StyleMelGAN TADEResBlock (a3t_smg_conv): v = bias + conv(x nearest-upsampled by `up`), then
    mode SMG_PLAIN: y = v (wt [taps*Cin][64]);  SMG_TADE: y = v[:, :64] * instance_norm(m upsampled by ux) + v[:, 64:] with
    stats [B][2][64] = mean | rstd of m (smg_stats);  SMG_GATE: y = softmax(v[:, :64], channels) (or sigmoid) * tanh(v[:, 64:])
    (+ R upsampled by ur) (both wt [taps*Cin][128]).  x fp32 [B*ceil(Tw/up)][Cin], Cin a multiple of 16; m / R [B*ceil(Tw/u)][64];
    y [B*Tw][64], overlapping neither x nor m; wt k-major (vocoder.pack_hifigan_conv), taps odd <= 9.  tiles: as hfg_conv."""
    Cin = x.shape[-1]
    N = 64 if mode == SMG_PLAIN else 128
    _ragged_f32("smg_conv", x, wt, bias, m, stats, R, y)
    if wt.dim() != 2 or wt.shape[1] != N or wt.shape[0] % Cin:
        raise ValueError(f"smg_conv: wt must be [taps*{Cin}][{N}], got {tuple(wt.shape)}")
    for name, t, u, C in (("x", x, up, Cin), ("m", m, ux, 64), ("R", R, ur, 64), ("y", y, 1, 64)):
        if t is not None and (u < 1 or t.shape[-1] != C or t.numel() != B * -(-Tw // u) * C):
            raise ValueError(f"smg_conv: {name} must be a contiguous fp32 [{B * -(-Tw // max(u, 1))}][{C}] tensor")
    if mode == SMG_TADE and (m is None or stats is None or stats.numel() != B * 128):
        raise ValueError(f"smg_conv: the TADE epilogue needs m and stats [{B}][2][64]")
    for name, o in (("x", x), ("m", m if mode == SMG_TADE else None)):      # other tiles read x[t +- halo] and m[t / ux]
        if o is not None and y.data_ptr() < o.data_ptr() + 4 * o.numel() and o.data_ptr() < y.data_ptr() + 4 * y.numel():
            raise ValueError(f"smg_conv: y overlaps {name}")
    if bias is not None and bias.numel() != N:
        raise ValueError(f"smg_conv: bias must have {N} entries")
    tp, nt = _tile_list("smg_conv", tiles, B, Tw)
    if nt < 0:
        return
    L.check(L.load().a3t_smg_conv(_ptr(x), _ptr(wt), _ptr(bias), _ptr(m), _ptr(stats), _ptr(R), _ptr(y), mode, int(bool(sigmoid)),
                                  tp, nt, B, Tw, Cin, N, wt.shape[0] // Cin, dil, up, ux, ur, _stream()), "smg_conv")


def smg_stats(x, stats, B, Tw, tiles=None, eps=1e-5, part=None):
    """stats [B][2][64] = mean | 1 / sqrt(biased variance + eps) per (row, channel) of x fp32 [B*Tw][64] over each row's own
    length (a3t_smg_stats; torch.nn.InstanceNorm1d).  Deterministic, and a row's result depends on nothing but the row.
    part: scratch of 128 floats per tile (allocated here when None).  tiles: as hfg_conv."""
    _ragged_f32("smg_stats", x, stats, part)
    if x.shape[-1] != 64 or x.numel() != B * Tw * 64 or stats.numel() != B * 128:
        raise ValueError(f"smg_stats: x must be [{B * Tw}][64] and stats [{B}][2][64]")
    tp, nt = _tile_list("smg_stats", tiles, B, Tw)
    if nt < 0:
        return
    need = 128 * (nt if tiles is not None else B * ((Tw + 255) // 256))
    if part is None:
        part = torch.empty(need, dtype=torch.float32, device=x.device)
    elif part.numel() < need:
        raise ValueError(f"smg_stats: part must hold {need} floats")
    L.check(L.load().a3t_smg_stats(_ptr(x), _ptr(part), _ptr(stats), eps, tp, nt, B, Tw, 64, _stream()), "smg_stats")


def reflect_pad_rows(x, y, pad, lens=None, mul=1):
    """x [T][C] or [B][T][C] (contiguous fp32) -> y [.., T + 2 pad, C], reflected like torch.nn.ReflectionPad1d (a3t_reflect_pad_rows).
    lens (device int32 [B]): row b is reflected at its own ends, its length being lens[b] * mul."""
    B, T, C = _rows_lens("reflect_pad_rows", x, lens)
    _ragged_f32("reflect_pad_rows", x, y)
    if y.numel() != B * (T + 2 * pad) * C:
        raise ValueError("reflect_pad_rows: shapes do not fit")
    if lens is None:
        rc = L.load().a3t_reflect_pad_rows(_ptr(x), _ptr(y), B, T, C, pad, _stream())
    else:
        rc = L.load().a3t_reflect_pad_rows_ragged(_ptr(x), _ptr(y), _ptr(lens), mul, B, T, C, pad, _stream())
    L.check(rc, "reflect_pad_rows")


def splice_spans(after, speech, speech_mask, spans, out, lens):
    """out[b][t] = after[b][t] inside spans[b], speech[b][t] for the other valid frames, 0 behind the row's length (the sum of
    its speech_mask, written to lens).  after / speech [B][Tin][C] fp32, speech_mask [B][Tin] bool / uint8, out [B][Tout][C]."""
    B, Tin, C = speech.shape
    if after.shape != speech.shape or speech_mask.numel() != B * Tin or spans.shape != (B, 2) or out.shape[0] != B \
            or out.shape[2] != C or lens.numel() != B:
        raise ValueError("splice_spans: shapes do not fit")
    for t in (after, speech, speech_mask, out):
        if not t.is_contiguous():
            raise ValueError("splice_spans: tensors must be contiguous")
    if after.dtype != torch.float32 or speech.dtype != torch.float32 or out.dtype != torch.float32 \
            or speech_mask.element_size() != 1:
        raise TypeError("splice_spans: after / speech / out fp32, speech_mask one byte per frame")
    L.check(L.load().a3t_splice_spans(_ptr(after), _ptr(speech), _ptr(speech_mask), _ptr(_i32(spans, "spans")), _ptr(out),
                                      _ptr(_i32(lens, "lens")), B, Tin, out.shape[1], C, _stream()), "splice_spans")


def splice_spans_multi(after, speech, speech_mask, spans, nspans, out, lens):
    """splice_spans with a list of spans per row: spans [B][S][2] int32, nspans [B] int32 (device); frame t of row b takes
    after[b][t] iff it lies in one of the row's first nspans[b] spans (a3t_splice_spans_multi)."""
    B, Tin, C = speech.shape
    if after.shape != speech.shape or speech_mask.numel() != B * Tin or spans.dim() != 3 or spans.shape[0] != B \
            or spans.shape[1] < 1 or spans.shape[2] != 2 or nspans.numel() != B or out.dim() != 3 or out.shape[0] != B \
            or out.shape[2] != C or lens.numel() != B:
        raise ValueError("splice_spans_multi: shapes do not fit")
    for t in (after, speech, speech_mask, out):
        if not t.is_contiguous():
            raise ValueError("splice_spans_multi: tensors must be contiguous")
    if after.dtype != torch.float32 or speech.dtype != torch.float32 or out.dtype != torch.float32 \
            or speech_mask.element_size() != 1:
        raise TypeError("splice_spans_multi: after / speech / out fp32, speech_mask one byte per frame")
    L.check(L.load().a3t_splice_spans_multi(_ptr(after), _ptr(speech), _ptr(speech_mask), _ptr(_i32(spans, "spans")),
                                            _ptr(_i32(nspans, "nspans")), _ptr(out), _ptr(_i32(lens, "lens")), B, Tin,
                                            out.shape[1], C, spans.shape[1], _stream()), "splice_spans_multi")


def gather_windows(src, table, dst):
    """dst [R][Wmax][C] row r = src[row, first:first + frames] with zeros behind, table [R][3] = {row, first frame, frames}
    (a3t_gather_windows).  src [B][T][C] fp32 on the device; `table` is a HOST array of integers: it is checked against the
    shapes here (0 <= row < B, 0 <= first, first + frames <= T, 0 <= frames <= Wmax), then copied to the device."""
    import numpy as np
    tab = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, 3))
    if src.dim() != 3 or dst.dim() != 3 or dst.shape[0] != tab.shape[0] or dst.shape[2] != src.shape[2] or tab.shape[0] < 1:
        raise ValueError("gather_windows: shapes do not fit")
    B, T, C = src.shape
    R, Wmax = dst.shape[0], dst.shape[1]
    if not src.is_contiguous() or not dst.is_contiguous() or src.dtype != torch.float32 or dst.dtype != torch.float32:
        raise ValueError("gather_windows: src and dst must be contiguous fp32")
    row, first, frames = tab[:, 0], tab[:, 1], tab[:, 2]
    if (row < 0).any() or (row >= B).any() or (first < 0).any() or (frames < 0).any() or (first + frames > T).any() \
            or (frames > Wmax).any():
        raise ValueError(f"gather_windows: a window of {tab.tolist()} leaves src {tuple(src.shape)} or dst {tuple(dst.shape)}")
    dev_tab = torch.from_numpy(tab.astype(np.int32)).to(src.device, non_blocking=True)
    L.check(L.load().a3t_gather_windows(_ptr(src), _ptr(dev_tab), _ptr(dst), R, T, Wmax, C, _stream()), "gather_windows")


def bias_act(x, bias, act, scale_=1.0):
    M, C = x.shape
    L.check(L.load().a3t_bias_act(_ptr(x), _ptr(bias), M, C, act, scale_, _stream()), "bias_act")


def duration_head(z, g, b, w, bias, logd, frames, eps=1e-12, offset=1.0):
    """logd[m] = LayerNorm(z[m]) . w + bias, frames[m] = clamp(round(exp(logd[m]) - offset), min=0) (int64)."""
    M, C = z.shape
    L.check(L.load().a3t_duration_head(_ptr(z), _ptr(g), _ptr(b), _ptr(w), _ptr(bias), _ptr(logd), _ptr(frames), M, C, eps,
                                       offset, _stream()), "duration_head")


def l2_normalize(x, y, eps=1e-12):
    B, n = x.shape
    L.check(L.load().a3t_l2_normalize(_ptr(x), _ptr(y), B, n, eps, _stream()), "l2_normalize")


def gst_conv_bn_relu(x, w, scale, shift, y, lens, k, s):
    """One GST reference-encoder layer: x [B][Tin][Fin][Cin] -> y [B][Tout][Fout][Cout] = relu(conv2d * scale + shift),
    w [k][k][Cin][Cout], stride s, padding (k - 1) // 2; lens: device int32 [B] (time lengths of x's rows) or None."""
    _ragged_f32("gst_conv_bn_relu", x, w, scale, shift, y)
    B, Tin, Fin, Cin = x.shape
    Cout, p = w.shape[3], (k - 1) // 2
    want = (B, (Tin + 2 * p - k) // s + 1, (Fin + 2 * p - k) // s + 1, Cout)
    if tuple(w.shape) != (k, k, Cin, Cout) or tuple(y.shape) != want or scale.numel() != Cout or shift.numel() != Cout or \
            (lens is not None and lens.numel() != B):
        raise ValueError("gst_conv_bn_relu: shapes do not fit")
    L.check(L.load().a3t_gst_conv_bn_relu(_ptr(x), _ptr(w), _ptr(scale), _ptr(shift), _ptr(y),
                                          _ptr(_i32(lens, "lens")) if lens is not None else None, B, Tin, Fin, Cin, Cout, k, s,
                                          _stream()), "gst_conv_bn_relu")


def gst_gru_stl(gi, w_hh, b_hh, lens, w_q, b_q, k_tok, v_tok, w_out, b_out, ref_embs, style, heads):
    """gi [B][T][3H] (input projections of every step) -> ref_embs [B][H] (or None) and style [B][d]: the GRU over each row's
    own lens[b] steps and the style-token attention (k_tok / v_tok [tokens][d])."""
    _ragged_f32("gst_gru_stl", gi, w_hh, b_hh, w_q, b_q, k_tok, v_tok, w_out, b_out, ref_embs, style)
    B, T, H3 = gi.shape
    H, (tokens, d) = H3 // 3, k_tok.shape
    if tuple(w_hh.shape) != (H3, H) or b_hh.numel() != H3 or tuple(w_q.shape) != (d, H) or tuple(v_tok.shape) != (tokens, d) \
            or tuple(w_out.shape) != (d, d) or tuple(style.shape) != (B, d) or \
            (ref_embs is not None and tuple(ref_embs.shape) != (B, H)) or (lens is not None and lens.numel() != B):
        raise ValueError("gst_gru_stl: shapes do not fit")
    L.check(L.load().a3t_gst_gru_stl(_ptr(gi), _ptr(w_hh), _ptr(b_hh), _ptr(_i32(lens, "lens")) if lens is not None else None,
                                     _ptr(w_q), _ptr(b_q), _ptr(k_tok), _ptr(v_tok), _ptr(w_out), _ptr(b_out), _ptr(ref_embs),
                                     _ptr(style), B, T, H, d, heads, tokens, _stream()), "gst_gru_stl")


def gst_add_style(hs, style, B, T, rows=None):
    """hs [B*T][d] (or [B][T][d]) += style [S][d]: row b takes style row rows[b] (device int32 [B]); without rows its own
    (S == B) or the only one (S == 1)."""
    _ragged_f32("gst_add_style", hs, style)
    d = hs.shape[-1]
    if hs.numel() != B * T * d or style.dim() != 2 or style.shape[1] != d or (rows is not None and rows.numel() != B):
        raise ValueError("gst_add_style: shapes do not fit")
    L.check(L.load().a3t_gst_add_style(_ptr(hs), _ptr(style), _ptr(_i32(rows, "rows")) if rows is not None else None, B, T, d,
                                       style.shape[0], _stream()), "gst_add_style")


def _lens_ptr(lens, B, what):
    if lens is None:
        return None
    if _i32(lens, "lens").numel() != B:
        raise ValueError(f"{what}: {lens.numel()} lengths for {B} rows")
    return _ptr(lens)


def fs2_variance_embed(hs, pitch, energy, wp, bp, we, be, lens, B, T):
    """hs [B*T][d] (or [B][T][d]) += pitch and energy embeddings of pitch / energy [B*T]: Conv1d(1 -> d) with weights wp
    [kp][d], we [ke][d] and biases bp, be [d]; lens (device int32 [B] or None): rows t >= lens[b] are left alone and the
    convolutions read zeros there."""
    _ragged_f32("fs2_variance_embed", hs, pitch, energy, wp, bp, we, be)
    d = hs.shape[-1]
    if hs.numel() != B * T * d or pitch.numel() != B * T or energy.numel() != B * T or wp.dim() != 2 or we.dim() != 2 or \
            wp.shape[1] != d or we.shape[1] != d or bp.numel() != d or be.numel() != d:
        raise ValueError("fs2_variance_embed: shapes do not fit")
    L.check(L.load().a3t_fs2_variance_embed(_ptr(hs), _ptr(pitch), _ptr(energy), _ptr(wp), _ptr(bp), _ptr(we), _ptr(be),
                                            _lens_ptr(lens, B, "fs2_variance_embed"), B, T, d, wp.shape[0], we.shape[0],
                                            _stream()), "fs2_variance_embed")


def length_offsets(frames, lens, alpha, offsets, frame_lens, scaled=None):
    """frames int64 [B][T] -> offsets int32 [B][T + 1] (exclusive prefix sums of the durations, scaled by alpha and rounded
    half to even when alpha != 1; entries behind lens[b] count as 0), frame_lens int32 [B], scaled int64 [B][T] (or None)."""
    B, T = frames.shape
    if frames.dtype != torch.int64 or not frames.is_contiguous() or tuple(_i32(offsets, "offsets").shape) != (B, T + 1) or \
            _i32(frame_lens, "frame_lens").numel() != B or \
            (scaled is not None and (scaled.dtype != torch.int64 or not scaled.is_contiguous() or scaled.numel() != B * T)):
        raise ValueError("length_offsets: shapes do not fit")
    L.check(L.load().a3t_length_offsets(_ptr(frames), _lens_ptr(lens, B, "length_offsets"), float(alpha), _ptr(offsets),
                                        _ptr(frame_lens), _ptr(scaled), B, T, _stream()), "length_offsets")


def length_expand(hs, offsets, lens, frame_lens, out, scale_=1.0):
    """The length regulator: hs [B][T][d], offsets / frame_lens of length_offsets -> out [B][Fp][d], row b holding scale_ *
    hs[b][token of frame f] for f < frame_lens[b] and 0 behind."""
    _ragged_f32("length_expand", hs, out)
    B, T, d = hs.shape
    if out.dim() != 3 or out.shape[0] != B or out.shape[2] != d or tuple(_i32(offsets, "offsets").shape) != (B, T + 1) or \
            _i32(frame_lens, "frame_lens").numel() != B:
        raise ValueError("length_expand: shapes do not fit")
    L.check(L.load().a3t_length_expand(_ptr(hs), _ptr(offsets), _lens_ptr(lens, B, "length_expand"), _ptr(frame_lens),
                                       _ptr(out), B, T, out.shape[1], d, scale_, _stream()), "length_expand")


def fs2_finish(before, post, after, lens=None, mean=None, std=None, denorm=None):
    """[B][F][C]: after = before + post (post None: before); denorm (or None) = after * std + mean; rows f >= lens[b]: 0."""
    _ragged_f32("fs2_finish", before, post, after, mean, std, denorm)
    B, F, C = before.shape
    for t in (post, after, denorm):
        if t is not None and t.shape != before.shape:
            raise ValueError("fs2_finish: shapes do not fit")
    for t in (mean, std):
        if t is not None and t.numel() != C:
            raise ValueError("fs2_finish: statistics do not fit")
    L.check(L.load().a3t_fs2_finish(_ptr(before), _ptr(post), _ptr(mean), _ptr(std), _ptr(after), _ptr(denorm),
                                    _lens_ptr(lens, B, "fs2_finish"), B, F, C, _stream()), "fs2_finish")


def fs2_mvn(x, mean, std, y):
    """y [M][C] = (x - mean) / std (GlobalMVN; mean / std [C] or None)."""
    _ragged_f32("fs2_mvn", x, mean, std, y)
    C = x.shape[-1]
    if y.shape != x.shape or any(t is not None and t.numel() != C for t in (mean, std)):
        raise ValueError("fs2_mvn: shapes do not fit")
    L.check(L.load().a3t_fs2_mvn(_ptr(x), _ptr(mean), _ptr(std), _ptr(y), x.numel() // C, C, _stream()), "fs2_mvn")


def dropout(x, y, p, key, scale=1.0):
    L.check(L.load().a3t_dropout(_ptr(x), _dt(x), _ptr(y), _dt(y), x.numel(), p, key, scale, _stream()), "dropout")


def dropout_bwd_cast(g, gm, p, key, colsum=None, colsum_scale=1.0):
    M, C = g.shape
    L.check(L.load().a3t_dropout_bwd_cast(_ptr(g), _ptr(gm), _dt(gm), _ptr(colsum), colsum_scale, M, C, p, key,
                                          _stream()), "dropout_bwd_cast")
