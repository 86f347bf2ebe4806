"""float64 references, a host restatement of the launchers' dispatch, and the case table for the row kernels of the Conformer
block (csrc/norm_reduce.hip, csrc/convmod_attn.hip, csrc/dwconv_vec.hip).

Three parts, used by tests/test_rowkernel_ref_host.py (no GPU) and tests/test_gpu_rowkernel_paths.py:

* `ref_*`: one plain float64 function per operation, evaluated on the operands the kernel receives (a bf16 operand is rounded
  first, then widened).  Every output comes back as `Out(ref, mag, intr)`: `mag` is the same formula with every term replaced by
  its absolute value (first-order error propagation for the non-linear steps), `intr` says whether the value passes through
  `__expf` / `expf` / `tanhf` on the device.
* `expected_path(op, shape, dtypes, aligned, options)`: what the launcher will do with that call -- a label such as
  `ln_bwd_row64<NP=3,DY16> pipeline` plus the launch facts (grid, loop trips, tiles per block, kernel instantiations, return code).
* `CASES`: small cases, each tagged with the label it is meant to reach and with L, the longest fp32 addition chain of that path
  per output (how it was read off the kernel is written next to the helpers `L_*` below).  `REQUIRED_LABELS` is the contract:
  the set of labels the table reaches must equal it.

Error bound of an fp32 output: |got - ref| <= ((L + 8) * 2^-23 + 2 * r) * mag, r = 0 unless `intr` (then r is the worst relative
error torch's fp32 CPU intrinsic shows on the case's own pre-activations).  bf16 outputs add one rounding, 2^-8 |ref|.  fp64
accumulators (`col_reduce`, the sums of `bn_act_bwd_a`): L * 2^-23 * mag with L the rows a lane adds in fp32 (at most 32).
"""
import collections
import math
import re
import zlib

import torch

EPS = 2.0 ** -23
EINVAL = -22
F64 = torch.float64
ACT_NONE, ACT_TANH, ACT_SWISH = 0, 2, 3
ACT_NAME = {ACT_NONE: "none", ACT_TANH: "tanh", ACT_SWISH: "swish"}
LN_MAXV = 24
DW_TT = 64
DW_KMAX = 31

Out = collections.namedtuple("Out", "ref mag intr")


def _out(ref, mag, intr=False):
    return Out(ref, mag, intr)


def bf16_round(t):
    """The value a bf16 store of t holds, as float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def widen(t):
    """An operand as the kernel reads it (bf16 / fp32 / uint8 / fp64 storage), in float64."""
    return t.to(F64)


# ----------------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------------
def ref_layernorm_fwd(x, g, b, eps):
    """y = (x - mean) * rstd * g + b per row; mean, rstd per row.  d rstd = -rstd^3 / 2 d var gives rstd's magnitude."""
    x, g, b = widen(x), widen(g), widen(b)
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    y = (x - mu) * rs * g + b
    mmu = x.abs().mean(1, keepdim=True)
    mvar = ((x.abs() + mmu) ** 2).mean(1, keepdim=True)
    mrs = rs + 0.5 * rs ** 3 * mvar
    my = (x.abs() + mmu) * mrs * g.abs() + b.abs()
    return dict(y=_out(y, my), mean=_out(mu[:, 0], mmu[:, 0]), rstd=_out(rs[:, 0], mrs[:, 0]))


def ref_layernorm_fwd_ragged(x, g, b, eps, lens, B, T):
    """The kernel comment (norm_reduce.hip): 'a row t >= lens[b] is stored as 0 ... without x being read', and mean / rstd of such a
    row are stored as 0 where they are asked for.  Rows in front of the length are the dense LayerNorm of that row: LayerNorm has no
    coupling between rows, so 'row b passed alone' is the dense reference on x[b, :lens[b]]."""
    D = x.shape[1]
    y, my = torch.zeros(B * T, D, dtype=F64), torch.zeros(B * T, D, dtype=F64)
    st = {k: [torch.zeros(B * T, dtype=F64), torch.zeros(B * T, dtype=F64)] for k in ("mean", "rstd")}
    for bb in range(B):
        n = max(0, min(T, int(lens[bb])))
        if n == 0:
            continue
        r = ref_layernorm_fwd(x[bb * T:bb * T + n], g, b, eps)
        y[bb * T:bb * T + n], my[bb * T:bb * T + n] = r["y"].ref, r["y"].mag
        for k in st:
            st[k][0][bb * T:bb * T + n], st[k][1][bb * T:bb * T + n] = r[k].ref, r[k].mag
    return dict(y=_out(y, my), mean=_out(*st["mean"]), rstd=_out(*st["rstd"]))


def ref_layernorm_bwd(dy, x, g, mean, rstd, dres=None, dxsum_scale=1.0, keep=None, drop_p=0.0):
    """dx = dres + rstd * (dy g - mean_row(dy g) - xhat mean_row(dy g xhat)); dgamma = sum_rows dy xhat, dbeta = sum_rows dy.  `dx` is
    never dropped; `dx16` (the bf16 copy) and `dxsum` (dxsum_scale * column sum) carry keep * dx / (1 - p) when drop_p > 0."""
    dy, x, g, mu, rs = widen(dy), widen(x), widen(g), widen(mean)[:, None], widen(rstd)[:, None]
    xh = (x - mu) * rs
    mxh = (x.abs() + mu.abs()) * rs
    dg = dy * g
    s1, s2 = dg.mean(1, keepdim=True), (dg * xh).mean(1, keepdim=True)
    ms1, ms2 = dg.abs().mean(1, keepdim=True), (dg.abs() * mxh).mean(1, keepdim=True)
    dx = rs * (dg - s1 - xh * s2)
    mdx = rs * (dg.abs() + ms1 + mxh * ms2)
    if dres is not None:
        dx, mdx = dx + widen(dres), mdx + widen(dres).abs()
    o, mo = dx, mdx
    if drop_p > 0.0:
        sc = widen(keep) / (1.0 - drop_p)
        o, mo = dx * sc, mdx * sc
    return dict(dx=_out(dx, mdx), dx16=_out(o, mo), dgamma=_out((dy * xh).sum(0), (dy.abs() * mxh).sum(0)),
                dbeta=_out(dy.sum(0), dy.abs().sum(0)), dxsum=_out(dxsum_scale * o.sum(0), abs(dxsum_scale) * mo.sum(0)))


def ref_col_reduce(x, mode, y=None, rowmask=None):
    """out0 = sum_rows x, out1 = sum_rows x^2 (mode 1) or sum_rows x y (mode 2), over the rows whose mask byte is non-zero.  x and
    y are the [M][C] views (the caller has applied `ld`)."""
    x = widen(x)
    if rowmask is not None:
        x = x * (rowmask != 0).to(F64)[:, None]
    r = dict(out0=_out(x.sum(0), x.abs().sum(0)))
    if mode == 1:
        r["out1"] = _out((x * x).sum(0), (x * x).sum(0))
    elif mode == 2:
        r["out1"] = _out((x * widen(y)).sum(0), (x * widen(y)).abs().sum(0))
    return r


def _act(bn, act):
    """act(bn), |d act / d bn| and whether an intrinsic is involved."""
    if act == ACT_SWISH:
        sg = torch.sigmoid(bn)
        return bn * sg, (sg * (1.0 + bn * (1.0 - sg))).abs(), True
    if act == ACT_TANH:
        t = torch.tanh(bn)
        return t, 1.0 - t * t, True
    return bn, torch.ones_like(bn), False


def ref_bn_act_fwd(z, stats, g, b, rmean, rvar, eps, momentum, training, act):
    """BatchNorm1d over the rows of z [M][C] from stats = (sum z, sum z^2) in fp64, then the activation.  Training: batch mean and
    biased variance normalise, the running statistics move by `momentum` towards the mean and the UNBIASED variance (M / (M - 1)).
    Eval: the running statistics normalise and stay."""
    z, g, b = widen(z), widen(g), widen(b)
    M, C = z.shape
    rm, rv = widen(rmean), widen(rvar)
    if training:
        mu = widen(stats)[:C] / M
        var = (widen(stats)[C:] / M - mu * mu).clamp_min(0.0)
        unb = var * M / (M - 1) if M > 1 else var
        nrm, nrv = (1.0 - momentum) * rm + momentum * mu, (1.0 - momentum) * rv + momentum * unb
        mrm, mrv = (1.0 - momentum) * rm.abs() + momentum * mu.abs(), (1.0 - momentum) * rv.abs() + momentum * unb
    else:
        mu, var = rm, rv
        nrm, nrv, mrm, mrv = rm, rv, rm.abs(), rv.abs()
    rs = 1.0 / torch.sqrt(var + eps)
    bn = (z - mu) * rs * g + b
    mbn = (z.abs() + mu.abs()) * rs * g.abs() + b.abs()
    y, dact, intr = _act(bn, act)
    my = mbn * dact + y.abs()
    return dict(y=_out(y, my, intr), mean=_out(mu, mu.abs()), rstd=_out(rs, rs), running_mean=_out(nrm, mrm),
                running_var=_out(nrv, mrv), pre=bn)


def _bn_dact(dy, bn, act):
    """dy * act'(bn) and its magnitude: (1 - sg) and (1 - t^2) count as 1 + sg, 1 + t^2."""
    if act == ACT_SWISH:
        sg = torch.sigmoid(bn)
        return dy * sg * (1.0 + bn * (1.0 - sg)), dy.abs() * sg * (1.0 + bn.abs() * (1.0 + sg)), True
    if act == ACT_TANH:
        t = torch.tanh(bn)
        return dy * (1.0 - t * t), dy.abs() * (1.0 + t * t), True
    return dy, dy.abs(), False


def ref_bn_act_bwd_a(dy, z, mean, rstd, g, b, act):
    """sums[0:C] = sum_rows d, sums[C:2C] = sum_rows d * zhat, d = dy * act'(bn)."""
    dy, z, mu, rs, g, b = (widen(t) for t in (dy, z, mean, rstd, g, b))
    zh, mzh = (z - mu) * rs, (z.abs() + mu.abs()) * rs
    bn = zh * g + b
    d, md, intr = _bn_dact(dy, bn, act)
    # act' is evaluated at a rounded bn: |dy| |act''| |d bn| with |act''| < 1 for both activations
    md = md + dy.abs() * (mzh * g.abs() + b.abs()) * (1.0 if act != ACT_NONE else 0.0)
    return dict(sums=_out(torch.cat([d.sum(0), (d * zh).sum(0)]), torch.cat([md.sum(0), (md * mzh).sum(0)]), intr), pre=bn)


def ref_bn_act_bwd_b(dy, z, mean, rstd, g, b, sums, dgamma0, dbeta0, training, act):
    """dz = g rstd (d - sums0 / M - zhat sums1 / M) in training, g rstd d in eval; dgamma += sums1, dbeta += sums0."""
    dy, z, mu, rs, g, b, sums = (widen(t) for t in (dy, z, mean, rstd, g, b, sums))
    M, C = z.shape
    zh, mzh = (z - mu) * rs, (z.abs() + mu.abs()) * rs
    bn = zh * g + b
    d, md, intr = _bn_dact(dy, bn, act)
    md = md + dy.abs() * (mzh * g.abs() + b.abs()) * (1.0 if act != ACT_NONE else 0.0)
    if training:
        d = d - sums[:C] / M - zh * sums[C:] / M
        md = md + sums[:C].abs() / M + mzh * sums[C:].abs() / M
    return dict(dz=_out(g * rs * d, g.abs() * rs * md, intr),
                dgamma=_out(widen(dgamma0) + sums[C:], widen(dgamma0).abs() + sums[C:].abs()),
                dbeta=_out(widen(dbeta0) + sums[:C], widen(dbeta0).abs() + sums[:C].abs()), pre=bn)


def _dw_shift(v, k, K):
    """v [B][T][C] -> v[t + k - pad], zero outside 0..T-1."""
    off, T = k - (K - 1) // 2, v.shape[1]
    out = torch.zeros_like(v)
    lo, hi = max(0, -off), min(T, T - off)
    if hi > lo:
        out[:, lo:hi] = v[:, lo + off:hi + off]
    return out


def ref_glu_dwconv_fwd(g, w, bias, B, T):
    """glu = a * sigmoid(b) for g = [a | b] ([B*T][2C]); z[t][c] = bias[c] + sum_k w[c][k] glu[t + k - pad][c], zero padding per
    utterance.  z is taken from the unrounded glu (the kernels convolve their fp32 window, not the stored copy)."""
    g, w, bias = widen(g), widen(w), widen(bias)
    C, K = w.shape
    a, gate = g[:, :C].view(B, T, C), g[:, C:].view(B, T, C)
    glu = a * torch.sigmoid(gate)
    z, mz = bias.expand(B, T, C).clone(), bias.abs().expand(B, T, C).clone()
    for k in range(K):
        sh = _dw_shift(glu, k, K)
        z += sh * w[:, k]
        mz += sh.abs() * w[:, k].abs()
    return dict(glu=_out(glu.reshape(B * T, C), glu.abs().reshape(B * T, C), True),
                z=_out(z.reshape(B * T, C), mz.reshape(B * T, C), True), pre=gate)


def ref_glu_dwconv_fwd_ragged(g, w, bias, lens, B, T):
    """The kernel comment (convmod_attn.hip): row b 'is computed as if it had been passed alone: a tap reads 0 for t >= n, glu and z
    are stored as 0 for n <= t < Tseq'."""
    C = w.shape[0]
    r = {k: [torch.zeros(B * T, C, dtype=F64), torch.zeros(B * T, C, dtype=F64)] for k in ("glu", "z")}
    pre = torch.zeros(B, T, C, dtype=F64)
    for bb in range(B):
        n = max(0, min(T, int(lens[bb])))
        if n == 0:
            continue
        d = ref_glu_dwconv_fwd(g[bb * T:bb * T + n], w, bias, 1, n)
        for k in r:
            r[k][0][bb * T:bb * T + n], r[k][1][bb * T:bb * T + n] = d[k].ref, d[k].mag
        pre[bb, :n] = d["pre"][0]
    return dict(glu=_out(*r["glu"], True), z=_out(*r["z"], True), pre=pre)


def ref_glu_dwconv_bwd(dz, g, glu, w, B, T):
    """dglu[t] = sum_k w[k] dz[t + pad - k]; da = dglu sig(b), db = dglu a sig(b) (1 - sig(b)); dW[c][k] = sum dz[t] glu[t + k - pad]
    with glu the stored operand; dbias = sum dz; dgsum = column sums of (da | db)."""
    dz, g, glu, w = widen(dz), widen(g), widen(glu), widen(w)
    C, K = w.shape
    dzb, glb = dz.view(B, T, C), glu.view(B, T, C)
    a, gate = g[:, :C].view(B, T, C), g[:, C:].view(B, T, C)
    dglu, mdglu = torch.zeros(B, T, C, dtype=F64), torch.zeros(B, T, C, dtype=F64)
    dW, mdW = torch.zeros(C, K, dtype=F64), torch.zeros(C, K, dtype=F64)
    for k in range(K):
        sh = _dw_shift(dzb, K - 1 - k, K)             # dz[t + pad - k]
        dglu += sh * w[:, k]
        mdglu += sh.abs() * w[:, k].abs()
        sh = _dw_shift(glb, k, K)
        dW[:, k] = (dzb * sh).sum((0, 1))
        mdW[:, k] = (dzb.abs() * sh.abs()).sum((0, 1))
    sb = torch.sigmoid(gate)
    da, db = dglu * sb, dglu * a * sb * (1.0 - sb)
    mda, mdb = mdglu * sb, mdglu * a.abs() * sb * (1.0 + sb)
    dg = torch.cat([da, db], -1).reshape(B * T, 2 * C)
    mdg = torch.cat([mda, mdb], -1).reshape(B * T, 2 * C)
    return dict(dg=_out(dg, mdg, True), dW=_out(dW, mdW), dbias=_out(dzb.sum((0, 1)), dzb.abs().sum((0, 1))),
                dgsum=_out(dg.sum(0), mdg.sum(0), True), pre=gate)


def ref_add_pos_bias(qkv, u, v, d):
    q = widen(qkv)[:, :d]
    u, v = widen(u), widen(v)
    return dict(qu=_out(q + u, q.abs() + u.abs()), qv=_out(q + v, q.abs() + v.abs()))


def ref_add_pos_bias_bwd(dqu, dqv):
    a, b = widen(dqu), widen(dqv)
    return dict(dq=_out(a + b, a.abs() + b.abs()))


def rel_shift_index(T):
    """Legacy rel_shift as a gather: idx[i][j] is the flat position in the compact BD [T][T] that score (i, j) reads, -1 where the
    shifted matrix holds the inserted zero (j == i + 1).  j <= i reads BD[i][T-1-i+j], j > i + 1 reads BD[i+1][j-i-2]."""
    i = torch.arange(T)[:, None]
    j = torch.arange(T)[None, :]
    idx = torch.where(j <= i, i * T + (T - 1 - i + j), (i + 1) * T + (j - i - 2))
    return torch.where(j == i + 1, torch.full_like(idx, -1), idx)


def rel_shift_gather(bd):
    """bd [..., T, T] -> shifted [..., T, T] by index gather."""
    T = bd.shape[-1]
    idx = rel_shift_index(T)
    flat = bd.reshape(*bd.shape[:-2], T * T)
    return torch.where(idx >= 0, flat[..., idx.clamp_min(0)], torch.zeros((), dtype=bd.dtype))


def ref_relpos_softmax_fwd(ac, bd, keymask, scale, keep=None, drop_p=0.0):
    """probs = softmax_j((ac + rel_shift(bd)) * scale) over the keys whose mask byte is set; masked keys and rows without any key
    hold 0.  ac, bd [B][H][T][T], keymask [B][T].  probs_drop = keep * probs / (1 - p)."""
    ac, bd = widen(ac), widen(bd)
    sh = rel_shift_gather(bd)
    s = (ac + sh) * scale
    ms = (ac.abs() + sh.abs()) * abs(scale)
    ok = (keymask != 0)[:, None, None, :].expand_as(s)
    sm = torch.where(ok, s, torch.full_like(s, -math.inf))
    mx = sm.max(-1, keepdim=True).values
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(sm - mx)
    den = e.sum(-1, keepdim=True)
    p = torch.where(den > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))
    # d p_j = p_j (d s_j - sum_k p_k d s_k), |d s| <= ms;  the exponent s - max is itself a rounded difference
    mp = p * (1.0 + 2.0 * ms + 2.0 * (p * ms).sum(-1, keepdim=True))
    r = dict(probs=_out(p, mp, True), pre=torch.where(ok, sm - mx, torch.zeros_like(s)))
    if drop_p > 0.0:
        sc = widen(keep) / (1.0 - drop_p)
        r["probs_drop"] = _out(p * sc, mp * sc, True)
    return r


def ref_relpos_softmax_fwd_ragged(ac, bd, lens, scale):
    """Row b alone at length n = lens[b]: keys j < n, the shift taken at n on the [n][n] corner of BD (row stride T), query rows
    i >= n and keys j >= n stored as 0."""
    B, H, T, _ = ac.shape
    p, mp, pre = (torch.zeros(B, H, T, T, dtype=F64) for _ in range(3))
    for b in range(B):
        n = max(0, min(T, int(lens[b])))
        if n == 0:
            continue
        r = ref_relpos_softmax_fwd(ac[b:b + 1, :, :n, :n], bd[b:b + 1, :, :n, :n], torch.ones(1, n, dtype=torch.uint8), scale)
        p[b, :, :n, :n], mp[b, :, :n, :n], pre[b, :, :n, :n] = r["probs"].ref[0], r["probs"].mag[0], r["pre"][0]
    return dict(probs=_out(p, mp, True), pre=pre)


def ref_relpos_softmax_bwd(probs, dprobs, scale, dbd0, keep=None, drop_p=0.0, rowscale=None, head_major=False):
    """ds = P (dP - sum_j P dP) * scale with P = probs * rowscale[row] and dP = keep * dprobs / (1 - p).  dbd is ds un-shifted into
    the compact BD layout: every element the scores read is written exactly once, BD[0][0..T-2] (read by no score) is written 0,
    and nothing else of `dbd0` (the buffer's previous contents) changes.  head_major: dbd is laid out [H][B][T][T]."""
    P, dP = widen(probs), widen(dprobs)
    B, H, T, _ = P.shape
    if rowscale is not None:
        P = P * widen(rowscale).view(B, H, T, 1)
    if drop_p > 0.0:
        dP = dP * widen(keep) / (1.0 - drop_p)
    s = (P * dP).sum(-1, keepdim=True)
    ms = (P.abs() * dP.abs()).sum(-1, keepdim=True)
    ds = P * (dP - s) * scale
    mds = P.abs() * (dP.abs() + ms) * abs(scale)
    idx = rel_shift_index(T)
    hit = idx >= 0
    dbd, mdbd = widen(dbd0).clone().reshape(B, H, T * T), torch.zeros(B, H, T * T, dtype=F64)
    dbd[..., :T - 1] = 0.0
    dbd[..., idx[hit]] = ds[..., hit]
    mdbd[..., idx[hit]] = mds[..., hit]
    dbd, mdbd = dbd.view(B, H, T, T), mdbd.view(B, H, T, T)
    if head_major:
        dbd, mdbd = dbd.transpose(0, 1).contiguous(), mdbd.transpose(0, 1).contiguous()
    return dict(ds=_out(ds, mds), dbd=_out(dbd, mdbd))


def intrinsic_error(kind, pre):
    """Worst relative error of torch's fp32 CPU sigmoid / tanh / exp on the fp32-rounded pre-activations of a case (the reference side
    of the allowance for the device intrinsic, which the bound doubles)."""
    p32 = pre.to(torch.float32)
    fn = dict(sigmoid=torch.sigmoid, tanh=torch.tanh, exp=torch.exp)[kind]
    a32, a64 = fn(p32).to(F64), fn(p32.to(F64))
    okk = (a64 != 0) & torch.isfinite(a64) & (a64.abs() > 1e-30)
    if not bool(okk.any()):
        return 0.0
    return float(((a32 - a64).abs()[okk] / a64.abs()[okk]).max())


def bound(out, L, kind, r_intr=0.0):
    """The tolerance of one output: see the module docstring."""
    if kind == "f64":
        return L * EPS * out.mag
    b = ((L + 8) * EPS + (2.0 * r_intr if out.intr else 0.0)) * out.mag
    if kind == "bf16":
        b = b + 2.0 ** -8 * out.ref.abs()
    return b


# ----------------------------------------------------------------------------------------------------------------------
# the launchers' dispatch, restated
# ----------------------------------------------------------------------------------------------------------------------
def _ln_v(D):
    for lim, v in ((64, 1), (128, 2), (256, 4), (384, 6), (512, 8)):
        if D <= lim:
            return v
    return LN_MAXV


def _kt(K):
    return 7 if K <= 7 else (15 if K <= 15 else DW_KMAX)


def _sm_nv(T):
    for lim, v in ((128, 2), (256, 4), (512, 8), (1152, 18), (2048, 32)):
        if T <= lim:
            return v
    return 0


def _sm_nc(T):
    return 1 if T <= 512 else (2 if T <= 1024 else (3 if T <= 1536 else 4))


def _cdiv(a, b):
    return (a + b - 1) // b


def _stride_loop(units, cap=4096, threads=256):
    blocks = min(cap, _cdiv(units, threads))
    return blocks, _cdiv(units, blocks * threads)


def _dw_chunks(cb, B, tiles_t, target):
    chunks = 1
    while cb * B * chunks < target and chunks < tiles_t:
        chunks += 1
    tpb = _cdiv(tiles_t, chunks)
    return _cdiv(tiles_t, tpb), tpb


def expected_path(op, shape, dtypes=None, aligned=True, options=None):
    """(label, facts) of one call.  shape / dtypes / options are dicts; `aligned` says whether every base pointer the launcher looks
    at is 16-byte aligned.  facts: rc (0 or EINVAL), grid, trips (loop iterations of the busiest thread or wave), trips_min,
    tiles_per_block, kernels [(name, template arguments)]."""
    s, dt, o = shape, dtypes or {}, options or {}
    bf = lambda k: dt.get(k, "f32") == "bf16"      # noqa: E731
    f = dict(rc=0, kernels=[])
    if op == "ln_fwd":
        M, D, ragged = s["M"], s["D"], bool(o.get("ragged"))
        if D > 64 * LN_MAXV or M <= 0:
            return "ln_fwd EINVAL", dict(f, rc=EINVAL)
        tag = (" ragged" if ragged else "") + (" y16" if bf("y") else "")
        if D % 128 == 0 and D <= 512 and aligned:
            f.update(grid=_cdiv(M, 8), trips=1, kernels=[("ln_fwd_vec_kernel", (D // 128, ragged))])
            return f"ln_fwd_vec<NQ={D // 128}>" + tag, f
        f.update(grid=_cdiv(M, 4), trips=1, kernels=[("ln_fwd_kernel", (_ln_v(D), ragged))])
        return f"ln_fwd<V={_ln_v(D)}>" + tag + (" misaligned" if D % 128 == 0 and D <= 512 else ""), f
    if op == "ln_bwd":
        M, D, drop = s["M"], s["D"], o.get("drop_p", 0.0)
        if D > 64 * LN_MAXV or M <= 0 or drop < 0 or drop >= 1:
            return "ln_bwd EINVAL", dict(f, rc=EINVAL)
        extra = ("" if o.get("dres", True) else " no-dres") + (" dx16" if o.get("dx16") else "") + (" dxsum" if o.get("dxsum") else "") \
            + (" drop" if drop > 0 else "")
        if D % 128 == 0 and D <= 512 and aligned:
            grid = min(_cdiv(M, 8), 512)
            stride = grid * 8
            f.update(grid=grid, trips=_cdiv(M, stride), trips_min=M // stride, kernels=[("ln_bwd_row64_kernel", (D // 128, bf("dy")))])
            lab = f"ln_bwd_row64<NP={D // 128}" + (",DY16>" if bf("dy") else ">")
            if f["trips"] > 1:
                lab += " pipeline"
            if M < 8:
                lab += " short-block"
            return lab + extra, f
        if drop > 0:
            return "ln_bwd EINVAL(drop on generic)", dict(f, rc=EINVAL)
        grid = min(_cdiv(M, 4), 2048)
        f.update(grid=grid, trips=_cdiv(M, grid * 4), trips_min=M // (grid * 4), kernels=[("ln_bwd_kernel", (_ln_v(D),))])
        return f"ln_bwd<V={_ln_v(D)}>" + (" dy16" if bf("dy") else "") + (" wrap" if f["trips"] > 1 else "") + extra, f
    if op == "col_reduce":
        M, C, ld, mode = s["M"], s["C"], s.get("ld", s["C"]), o.get("mode", 0)
        if M <= 0 or C <= 0:
            return "col_reduce EINVAL", dict(f, rc=EINVAL)
        if _cdiv(M, 256) > 65535:
            return "col_reduce EINVAL(grid.y)", dict(f, rc=EINVAL)
        rows = min(M, 256)
        size = (" M<16" if M < 16 else "") + (" blocks>1" if M > 256 else "")
        f.update(grid=(_cdiv(C, 64), _cdiv(M, 256)))
        why = [w for w, hit in (("bf16 x", bf("x")), ("rowmask", bool(o.get("rowmask"))), ("C%64", C % 64 != 0), ("ld%4", ld % 4 != 0),
                                ("misaligned", not aligned)) if hit]
        if not why:
            f.update(trips=_cdiv(rows, 16), kernels=[("col_reduce_vec_kernel", ())])
            return f"col_reduce_vec mode={mode}" + size, f
        f.update(trips=_cdiv(rows, 4), kernels=[("col_reduce_kernel", ())])
        return f"col_reduce generic({','.join(why)}) mode={mode}" + size, f
    if op == "f64_to_f32_add":
        f.update(grid=_cdiv(s["n"], 256), trips=1, kernels=[("f64_to_f32_add_kernel", ())])
        return "f64_to_f32_add", f
    if op == "bn_act_fwd":
        M, C = s["M"], s["C"]
        vec = C % 4 == 0 and aligned
        n = M * C
        grid, trips = _stride_loop(n // 4 if vec else n)
        f.update(grid=grid, trips=trips, kernels=[("bn_finalize_kernel", ()), ("bn_act_fwd_kernel", ())])
        return (f"bn_act_fwd {'vec' if vec else 'generic'} {'y16' if bf('y') else 'f32'} {ACT_NAME[o.get('act', ACT_NONE)]} "
                f"{'train' if o.get('training', True) else 'eval'}" + (" wrap" if trips > 1 else "") + (" M=2" if M == 2 else "")), f
    if op == "bn_act_bwd_a":
        M, C = s["M"], s["C"]
        if _cdiv(M, 256) > 65535:
            return "bn_act_bwd_a EINVAL(grid.y)", dict(f, rc=EINVAL)
        f.update(grid=(_cdiv(C, 64), _cdiv(M, 256)))
        if bf("dy"):
            why = "dy16"
        elif C % 64 != 0:
            why = "C%64"
        elif not aligned:
            why = "misaligned"
        else:
            f.update(trips=_cdiv(min(M, 256), 16), kernels=[("bn_act_bwd_a_vec_kernel", ())])
            return "bn_act_bwd_a vec " + ACT_NAME[o.get("act", ACT_NONE)], f
        f.update(trips=_cdiv(min(M, 256), 4), kernels=[("bn_act_bwd_a_kernel", ())])
        return f"bn_act_bwd_a generic({why}) " + ACT_NAME[o.get("act", ACT_NONE)], f
    if op == "bn_act_bwd_b":
        M, C = s["M"], s["C"]
        n = M * C
        why = "dy16" if bf("dy") else ("C%4" if C % 4 != 0 else ("misaligned" if not aligned else ""))
        grid, trips = _stride_loop(n if why else n // 4)
        f.update(grid=grid, trips=trips, kernels=[("bn_act_bwd_b_kernel", ())])
        return (("bn_act_bwd_b " + (f"generic({why})" if why else "vec") + " " + ACT_NAME[o.get("act", ACT_NONE)]
                 + (" train" if o.get("training", True) else " eval")) + (" wrap" if trips > 1 else "")), f
    if op in ("glu_dwconv_fwd", "glu_dwconv_bwd"):
        B, T, C, K, ragged = s["B"], s["T"], s["C"], s["K"], bool(o.get("ragged"))
        if K > DW_KMAX or K <= 0 or K % 2 == 0 or T <= 0 or B <= 0 or C <= 0:
            return op + " EINVAL", dict(f, rc=EINVAL)
        tiles_t, cb, kt, pad = _cdiv(T, DW_TT), _cdiv(C, 64), _kt(K), (K - 1) // 2
        kk = " K==KT" if K == kt else " K<KT"
        tcls = " T=1" if T == 1 else (" T=pad" if T == pad else (f" T={T}" if T in (63, 64, 65) and not ragged else ""))
        if op == "glu_dwconv_fwd":
            if B * tiles_t > 65535:
                return "glu_dwconv_fwd EINVAL(grid.y)", dict(f, rc=EINVAL)
            f.update(grid=(cb, B * tiles_t), trips=1, tiles_per_block=1)
            if not ragged and bf("g") and bf("glu") and C % 64 == 0 and aligned:
                f["kernels"] = [("glu_dwconv_fwd_vec_kernel", (kt,))]
                return f"glu_dwconv_fwd_vec<KT={kt}>" + kk + tcls, f
            f["kernels"] = [("glu_dwconv_fwd_kernel", (kt, ragged))]
            return (f"glu_dwconv_fwd<KT={kt}>" + kk + (" ragged" if ragged else "") + (" bf16" if bf("g") or bf("glu") else "")
                    + tcls), f
        vec = bf("g") and bf("glu") and bf("dg") and C % 64 == 0 and aligned
        chunks, tpb = _dw_chunks(cb, B, tiles_t, 640 if vec else 1024)
        if B * chunks > 65535:
            return "glu_dwconv_bwd EINVAL(grid.y)", dict(f, rc=EINVAL)
        f.update(grid=(cb, B * chunks), trips=tpb, trips_min=tiles_t - (chunks - 1) * tpb, tiles_per_block=tpb, chunks=chunks,
                 kernels=[("glu_dwconv_bwd_vec_kernel" if vec else "glu_dwconv_bwd_kernel", (kt,))])
        return ((f"glu_dwconv_bwd_vec<KT={kt}>" if vec else f"glu_dwconv_bwd<KT={kt}>") + kk + (" tpb>1" if tpb > 1 else "")
                + (" bf16" if not vec and (bf("g") or bf("glu") or bf("dg")) else "") + (" dgsum" if o.get("dgsum") else "")), f
    if op in ("add_pos_bias", "add_pos_bias_bwd"):
        M, d = s["M"], s["d"]
        n = M * d
        if bf("x") and d % 8 == 0 and aligned:
            grid, trips = _stride_loop(n // 8)
            f.update(grid=grid, trips=trips, kernels=[(op + "_bf16_kernel", ())])
            return op + "_bf16 vec" + (" wrap" if trips > 1 else ""), f
        grid, trips = _stride_loop(n)
        f.update(grid=grid, trips=trips, kernels=[(op + "_kernel", ())])
        why = "f32" if not bf("x") else ("bf16 d%8" if d % 8 else "bf16 misaligned")
        return f"{op} generic({why})" + (" wrap" if trips > 1 else ""), f
    if op == "relpos_softmax_fwd":
        B, H, T, ragged, drop = s["B"], s["H"], s["T"], bool(o.get("ragged")), o.get("drop_p", 0.0)
        if drop < 0 or drop >= 1 or (ragged and (bf("s") or bf("p"))):
            return "relpos_softmax_fwd EINVAL", dict(f, rc=EINVAL)
        nrows = B * H * T
        masks = o.get("masks")
        tag = (" rows%4" if nrows % 4 else "") + (f" keymask({','.join(masks)})" if masks else "") + (" drop" if drop > 0 else "")
        f.update(grid=_cdiv(nrows, 4))
        if not ragged and bf("s") and bf("p") and T % 8 == 0 and T <= 2048 and aligned:
            f.update(trips=1, kernels=[("relpos_softmax_fwd_bf16_kernel", (_sm_nc(T),))])
            return f"relpos_softmax_fwd_bf16<NC={_sm_nc(T)}>" + tag, f
        nv = _sm_nv(T)
        f.update(trips=1 if nv else _cdiv(T, 64), kernels=[("relpos_softmax_fwd_kernel", (nv, ragged))])
        return (f"relpos_softmax_fwd<NV={nv}>" + (" ragged" if ragged else "") + (" bf16" if bf("s") or bf("p") else "") + tag), f
    if op == "relpos_softmax_bwd":
        B, H, T, drop = s["B"], s["H"], s["T"], o.get("drop_p", 0.0)
        if drop < 0 or drop >= 1:
            return "relpos_softmax_bwd EINVAL", dict(f, rc=EINVAL)
        stored = drop > 0 and bool(o.get("stored_mask"))
        regen = drop > 0 and not stored
        tag = (" head_major" if o.get("head_major") else "") + (" inplace" if o.get("inplace") else "") \
            + (" rowscale" if o.get("rowscale") else "") + (" drop(stored)" if stored else "") + (" drop(regen)" if regen else "")
        f.update(grid=_cdiv(B * H * T, 4))
        if bf("p") and bf("dp") and bf("o") and T % 8 == 0 and T <= 2048 and aligned and not o.get("inplace"):
            f.update(trips=1, kernels=[("relpos_softmax_bwd_bf16_kernel", (_sm_nc(T),))])
            return f"relpos_softmax_bwd_bf16<NC={_sm_nc(T)}>" + tag, f
        if regen or o.get("rowscale"):
            return "relpos_softmax_bwd EINVAL(" + ("regenerated mask" if regen else "rowscale") + " on generic)", dict(f, rc=EINVAL)
        nv = _sm_nv(T)
        f.update(trips=1 if nv else _cdiv(T, 64), kernels=[("relpos_softmax_bwd_kernel", (nv,))])
        return f"relpos_softmax_bwd<NV={nv}>" + (" bf16" if bf("p") or bf("dp") or bf("o") else "") + tag, f
    raise KeyError(op)


def demangle(sym):
    """'_Z19ln_bwd_row64_kernelILi3ELb1EEv...' -> ('ln_bwd_row64_kernel', (3, True)); plain kernels give ()."""
    m = re.match(r"_Z(\d+)", sym)
    n = int(m.group(1))
    name, rest = sym[m.end():m.end() + n], sym[m.end() + n:]
    args = []
    if rest.startswith("I"):
        for kind, val in re.findall(r"L([ib])(\d+)E", rest[1:rest.index("EE") + 1]):
            args.append(bool(int(val)) if kind == "b" else int(val))
    return name, tuple(args)


# ----------------------------------------------------------------------------------------------------------------------
# L: the longest fp32 addition chain per output, as read off the kernels
# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm forward: a lane adds its V (generic) or 4 NQ (vector, four per float4) values, then 6 (5) __shfl_xor steps.
def L_ln_fwd(V=None, NQ=None):
    return V + 6 if V else 4 * NQ + 5


# LayerNorm backward: dx as forward (2 NP values per lane, 6 shuffles).  Column sums: one add per row of the wave (`trips`), the LDS
# sum over the block's waves (7 adds for eight waves, 3 for four), one atomic per block on every address (`grid`).
def L_ln_bwd(facts, V=None, NP=None):
    cols = facts["trips"] + (7 if NP else 3) + facts["grid"]
    return dict(dx=(2 * NP if NP else V) + 6, dx16=(2 * NP if NP else V) + 6, dgamma=cols, dbeta=cols, dxsum=cols)


# Depthwise conv: K multiply-adds onto the bias (forward) / onto 0 (dglu).  Weight gradients: 16 outputs per thread and tile times
# tiles per block, 4 row groups through LDS, one atomic per block of the same channels (grid.y).
def L_dw_bwd(facts, K):
    cols = 16 * facts["tiles_per_block"] + 4 + facts["grid"][1]
    return dict(dg=K, dW=cols, dbias=cols, dgsum=cols)


# Softmax: NV (8 NC) adds per lane, 6 shuffles; NV = 0 loops ceil(T / 64) times.
def L_sm(facts):
    name, targs = facts["kernels"][0]
    per_lane = 8 * targs[0] if "bf16" in name else (targs[0] or facts["trips"])
    return per_lane + 6


def case_L(case):
    """L per output of a case (a dict, or one number for every output)."""
    op, f = case["op"], case["facts"]
    if op == "ln_fwd":
        name, targs = f["kernels"][0]
        return L_ln_fwd(NQ=targs[0]) if "vec" in name else L_ln_fwd(V=targs[0])
    if op == "ln_bwd":
        name, targs = f["kernels"][0]
        return L_ln_bwd(f, NP=targs[0]) if "row64" in name else L_ln_bwd(f, V=targs[0])
    if op == "col_reduce":
        return min(32, f["trips"])           # rows a lane adds in fp32 before it spills into its fp64 accumulator
    if op == "bn_act_bwd_a":
        return min(32, f["trips"])           # the same scheme (sums are fp64: the bound is L 2^-23 mag here too)
    if op in ("bn_act_fwd", "f64_to_f32_add", "add_pos_bias", "add_pos_bias_bwd"):
        return 1                             # element-wise: no chain beyond the expression itself
    if op == "bn_act_bwd_b":
        return 2                             # d - sums0 / M - zhat sums1 / M
    if op == "glu_dwconv_fwd":
        return dict(glu=1, z=case["shape"]["K"])
    if op == "glu_dwconv_bwd":
        return L_dw_bwd(f, case["shape"]["K"])
    if op in ("relpos_softmax_fwd", "relpos_softmax_bwd"):
        return L_sm(f)
    raise KeyError(op)


# ----------------------------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------------------------
RAGGED_LENS_70 = (0, 1, 70, 64, 65)          # 0, 1, T, a 64-frame tile edge and one past it


def _c(cid, op, label, shape, dtypes=None, aligned=True, **options):
    return dict(id=cid, op=op, label=label, shape=shape, dtypes=dtypes or {}, aligned=aligned, options=options)


def _ln_cases():
    cs = []
    for nq in (1, 2, 3, 4):
        D = 128 * nq
        cs.append(_c(f"ln_fwd_vec{nq}", "ln_fwd", f"ln_fwd_vec<NQ={nq}>", dict(M=37, D=D)))
        cs.append(_c(f"ln_fwd_vec{nq}_ragged", "ln_fwd", f"ln_fwd_vec<NQ={nq}> ragged", dict(M=350, D=D), ragged=True, B=5, T=70,
                     lens=RAGGED_LENS_70))
    for v, D in ((1, 40), (2, 100), (4, 200), (6, 300), (8, 500), (24, 1000)):
        cs.append(_c(f"ln_fwd_v{v}", "ln_fwd", f"ln_fwd<V={v}>", dict(M=37, D=D)))
        cs.append(_c(f"ln_fwd_v{v}_ragged", "ln_fwd", f"ln_fwd<V={v}> ragged", dict(M=350, D=D), ragged=True, B=5, T=70,
                     lens=RAGGED_LENS_70))
    cs.append(_c("ln_fwd_vec3_y16", "ln_fwd", "ln_fwd_vec<NQ=3> y16", dict(M=37, D=384), dict(y="bf16")))
    cs.append(_c("ln_fwd_v6_y16", "ln_fwd", "ln_fwd<V=6> y16", dict(M=37, D=300), dict(y="bf16")))
    cs.append(_c("ln_fwd_misaligned", "ln_fwd", "ln_fwd<V=6> misaligned", dict(M=37, D=384), aligned=False))
    cs.append(_c("ln_fwd_v24_1536", "ln_fwd", "ln_fwd<V=24>", dict(M=9, D=1536)))
    for np_ in (1, 2, 3, 4):
        for dy16 in (False, True):
            cs.append(_c(f"ln_bwd_r64_{np_}{'_dy16' if dy16 else ''}", "ln_bwd", f"ln_bwd_row64<NP={np_}{',DY16' if dy16 else ''}> dxsum",
                         dict(M=77, D=128 * np_), dict(dy="bf16" if dy16 else "f32"), dxsum=True))
    # 4096 rows fill the 512 x 8 waves once: M = 4099 + 4 leaves waves with two rows, waves with one, and M % 8 != 0
    cs.append(_c("ln_bwd_pipeline", "ln_bwd", "ln_bwd_row64<NP=3> pipeline dxsum", dict(M=4103, D=384), dxsum=True))
    cs.append(_c("ln_bwd_pipeline_dy16", "ln_bwd", "ln_bwd_row64<NP=3,DY16> pipeline dx16 dxsum", dict(M=4103, D=384), dict(dy="bf16"),
                 dxsum=True, dx16=True))
    cs.append(_c("ln_bwd_pipeline3", "ln_bwd", "ln_bwd_row64<NP=1> pipeline dxsum", dict(M=8197, D=128), dxsum=True))
    cs.append(_c("ln_bwd_short", "ln_bwd", "ln_bwd_row64<NP=3> short-block dxsum", dict(M=5, D=384), dxsum=True))
    cs.append(_c("ln_bwd_nodres", "ln_bwd", "ln_bwd_row64<NP=3> no-dres", dict(M=77, D=384), dres=False))
    cs.append(_c("ln_bwd_drop", "ln_bwd", "ln_bwd_row64<NP=3> dx16 dxsum drop", dict(M=333, D=384), dx16=True, dxsum=True, drop_p=0.1,
                 drop_key=0x9E3779B9))
    cs.append(_c("ln_bwd_drop_pipeline", "ln_bwd", "ln_bwd_row64<NP=3,DY16> pipeline dx16 dxsum drop", dict(M=4103, D=384), dict(dy="bf16"),
                 dx16=True, dxsum=True, drop_p=0.1, drop_key=12345))
    for v, D in ((1, 40), (2, 100), (4, 200), (6, 300), (8, 500), (24, 1000)):
        for dy16 in (False, True):
            cs.append(_c(f"ln_bwd_v{v}{'_dy16' if dy16 else ''}", "ln_bwd", f"ln_bwd<V={v}>{' dy16' if dy16 else ''} dx16 dxsum",
                         dict(M=77, D=D), dict(dy="bf16" if dy16 else "f32"), dx16=True, dxsum=True))
    cs.append(_c("ln_bwd_wrap", "ln_bwd", "ln_bwd<V=1> wrap dxsum", dict(M=8199, D=24), dxsum=True))
    cs.append(_c("ln_bwd_misaligned", "ln_bwd", "ln_bwd<V=6> dxsum", dict(M=77, D=384), aligned=False, dxsum=True))
    cs.append(_c("ln_bwd_drop_generic", "ln_bwd", "ln_bwd EINVAL(drop on generic)", dict(M=77, D=300), drop_p=0.1, drop_key=1))
    return cs


def _col_bn_cases():
    cs = []
    cs.append(_c("col_vec_m0", "col_reduce", "col_reduce_vec mode=0", dict(M=100, C=128)))
    cs.append(_c("col_vec_m1", "col_reduce", "col_reduce_vec mode=1 M<16", dict(M=13, C=64), mode=1))
    cs.append(_c("col_vec_m2", "col_reduce", "col_reduce_vec mode=2 blocks>1", dict(M=777, C=128, ld=132), mode=2))
    cs.append(_c("col_gen_bf16", "col_reduce", "col_reduce generic(bf16 x) mode=0 blocks>1", dict(M=777, C=128), dict(x="bf16")))
    cs.append(_c("col_gen_mask", "col_reduce", "col_reduce generic(rowmask) mode=1 blocks>1", dict(M=777, C=128), mode=1, rowmask=True))
    cs.append(_c("col_gen_c", "col_reduce", "col_reduce generic(C%64) mode=2", dict(M=100, C=52), mode=2))
    cs.append(_c("col_gen_ld", "col_reduce", "col_reduce generic(ld%4) mode=2", dict(M=100, C=64, ld=67), mode=2))
    cs.append(_c("col_gen_misaligned", "col_reduce", "col_reduce generic(misaligned) mode=1 M<16", dict(M=7, C=64), aligned=False, mode=1))
    cs.append(_c("f64_add", "f64_to_f32_add", "f64_to_f32_add", dict(n=300)))
    for act in (ACT_NONE, ACT_SWISH, ACT_TANH):
        cs.append(_c(f"bn_fwd_vec_{ACT_NAME[act]}", "bn_act_fwd", f"bn_act_fwd vec f32 {ACT_NAME[act]} train", dict(M=203, C=132), act=act))
    cs.append(_c("bn_fwd_vec_eval", "bn_act_fwd", "bn_act_fwd vec f32 swish eval", dict(M=203, C=132), act=ACT_SWISH, training=False))
    cs.append(_c("bn_fwd_vec_y16", "bn_act_fwd", "bn_act_fwd vec y16 swish train", dict(M=203, C=132), dict(y="bf16"), act=ACT_SWISH))
    cs.append(_c("bn_fwd_vec_y16_eval", "bn_act_fwd", "bn_act_fwd vec y16 tanh eval", dict(M=203, C=132), dict(y="bf16"), act=ACT_TANH,
                 training=False))
    cs.append(_c("bn_fwd_gen", "bn_act_fwd", "bn_act_fwd generic f32 swish train", dict(M=203, C=50), act=ACT_SWISH))
    cs.append(_c("bn_fwd_gen_eval", "bn_act_fwd", "bn_act_fwd generic f32 tanh eval", dict(M=203, C=50), act=ACT_TANH, training=False))
    cs.append(_c("bn_fwd_gen_y16", "bn_act_fwd", "bn_act_fwd generic y16 none train", dict(M=203, C=50), dict(y="bf16"), act=ACT_NONE))
    cs.append(_c("bn_fwd_gen_y16_eval", "bn_act_fwd", "bn_act_fwd generic y16 swish eval", dict(M=203, C=50), dict(y="bf16"), act=ACT_SWISH,
                 training=False))
    cs.append(_c("bn_fwd_misaligned", "bn_act_fwd", "bn_act_fwd generic f32 none eval", dict(M=203, C=132), aligned=False, act=ACT_NONE,
                 training=False))
    cs.append(_c("bn_fwd_m2", "bn_act_fwd", "bn_act_fwd vec f32 swish train M=2", dict(M=2, C=132), act=ACT_SWISH))
    # 4096 blocks x 256 threads: the smallest M * C over the cap with C = 12 (16-byte lanes) and C = 6 (generic)
    cs.append(_c("bn_fwd_vec_wrap", "bn_act_fwd", "bn_act_fwd vec f32 swish train wrap", dict(M=349526, C=12), act=ACT_SWISH))
    cs.append(_c("bn_fwd_gen_wrap", "bn_act_fwd", "bn_act_fwd generic f32 swish train wrap", dict(M=174763, C=6), act=ACT_SWISH))
    cs.append(_c("bn_bwda_vec", "bn_act_bwd_a", "bn_act_bwd_a vec swish", dict(M=777, C=128), act=ACT_SWISH))
    cs.append(_c("bn_bwda_vec_tanh", "bn_act_bwd_a", "bn_act_bwd_a vec tanh", dict(M=203, C=64), act=ACT_TANH))
    cs.append(_c("bn_bwda_gen_c", "bn_act_bwd_a", "bn_act_bwd_a generic(C%64) swish", dict(M=777, C=132), act=ACT_SWISH))
    cs.append(_c("bn_bwda_gen_dy16", "bn_act_bwd_a", "bn_act_bwd_a generic(dy16) none", dict(M=777, C=128), dict(dy="bf16"), act=ACT_NONE))
    cs.append(_c("bn_bwdb_vec", "bn_act_bwd_b", "bn_act_bwd_b vec swish train", dict(M=203, C=132), act=ACT_SWISH))
    cs.append(_c("bn_bwdb_vec_eval", "bn_act_bwd_b", "bn_act_bwd_b vec tanh eval", dict(M=203, C=132), act=ACT_TANH, training=False))
    cs.append(_c("bn_bwdb_gen_c", "bn_act_bwd_b", "bn_act_bwd_b generic(C%4) swish train", dict(M=203, C=50), act=ACT_SWISH))
    cs.append(_c("bn_bwdb_gen_dy16", "bn_act_bwd_b", "bn_act_bwd_b generic(dy16) none train", dict(M=203, C=132), dict(dy="bf16"),
                 act=ACT_NONE))
    cs.append(_c("bn_bwdb_vec_wrap", "bn_act_bwd_b", "bn_act_bwd_b vec swish train wrap", dict(M=349526, C=12), act=ACT_SWISH))
    cs.append(_c("bn_bwdb_gen_wrap", "bn_act_bwd_b", "bn_act_bwd_b generic(C%4) swish train wrap", dict(M=174763, C=6), act=ACT_SWISH))
    return cs


def _dw_cases():
    cs = []
    bf3 = dict(g="bf16", glu="bf16", dg="bf16")
    for kt, klo in ((7, 5), (15, 9), (31, 17)):
        for K in (kt, klo):
            kk = "K==KT" if K == kt else "K<KT"
            cs.append(_c(f"dw_fwd_k{K}", "glu_dwconv_fwd", f"glu_dwconv_fwd<KT={kt}> {kk}", dict(B=2, T=100, C=50, K=K)))
            cs.append(_c(f"dw_fwd_k{K}_ragged", "glu_dwconv_fwd", f"glu_dwconv_fwd<KT={kt}> {kk} ragged", dict(B=5, T=70, C=50, K=K),
                         ragged=True, lens=RAGGED_LENS_70))
            cs.append(_c(f"dw_fwd_vec_k{K}", "glu_dwconv_fwd", f"glu_dwconv_fwd_vec<KT={kt}> {kk}", dict(B=2, T=100, C=128, K=K), bf3))
    cs.append(_c("dw_fwd_bf16_gen", "glu_dwconv_fwd", "glu_dwconv_fwd<KT=15> K==KT bf16", dict(B=2, T=100, C=50, K=15), bf3))
    cs.append(_c("dw_fwd_t1", "glu_dwconv_fwd", "glu_dwconv_fwd<KT=31> K==KT T=1", dict(B=3, T=1, C=50, K=31)))
    cs.append(_c("dw_fwd_tpad", "glu_dwconv_fwd", "glu_dwconv_fwd_vec<KT=31> K==KT T=pad", dict(B=3, T=15, C=64, K=31), bf3))
    cs.append(_c("dw_fwd_t63", "glu_dwconv_fwd", "glu_dwconv_fwd<KT=7> K==KT T=63", dict(B=2, T=63, C=70, K=7)))
    cs.append(_c("dw_fwd_t64", "glu_dwconv_fwd", "glu_dwconv_fwd_vec<KT=15> K==KT T=64", dict(B=2, T=64, C=64, K=15), bf3))
    cs.append(_c("dw_fwd_t65", "glu_dwconv_fwd", "glu_dwconv_fwd<KT=31> K==KT T=65", dict(B=2, T=65, C=70, K=31)))
    cs.append(_c("dw_fwd_grid", "glu_dwconv_fwd", "glu_dwconv_fwd EINVAL(grid.y)", dict(B=65536, T=1, C=1, K=1)))
    for kt in (7, 15, 31):
        cs.append(_c(f"dw_bwd_k{kt}", "glu_dwconv_bwd", f"glu_dwconv_bwd<KT={kt}> K==KT dgsum", dict(B=2, T=100, C=50, K=kt), dgsum=True))
        cs.append(_c(f"dw_bwd_vec_k{kt}", "glu_dwconv_bwd", f"glu_dwconv_bwd_vec<KT={kt}> K==KT dgsum", dict(B=2, T=100, C=128, K=kt), bf3,
                     dgsum=True))
    cs.append(_c("dw_bwd_klo", "glu_dwconv_bwd", "glu_dwconv_bwd<KT=15> K<KT", dict(B=2, T=100, C=50, K=9)))
    cs.append(_c("dw_bwd_vec_klo", "glu_dwconv_bwd", "glu_dwconv_bwd_vec<KT=31> K<KT", dict(B=2, T=100, C=64, K=17), bf3))
    cs.append(_c("dw_bwd_bf16_gen", "glu_dwconv_bwd", "glu_dwconv_bwd<KT=7> K==KT bf16 dgsum", dict(B=2, T=100, C=50, K=7), bf3, dgsum=True))
    for kt in (7, 31):
        # generic: C = 50 -> one channel block, 512 utterances x 3 tiles -> chunks 2: blocks of 2 tiles and of 1 (partial) tile
        cs.append(_c(f"dw_bwd_tpb_k{kt}", "glu_dwconv_bwd", f"glu_dwconv_bwd<KT={kt}> K==KT tpb>1" + (" dgsum" if kt == 7 else ""),
                     dict(B=512, T=130, C=50, K=kt), dgsum=kt == 7))
        # vector: 320 utterances x 3 tiles -> chunks 2
        cs.append(_c(f"dw_bwd_vec_tpb_k{kt}", "glu_dwconv_bwd", f"glu_dwconv_bwd_vec<KT={kt}> K==KT tpb>1" + (" dgsum" if kt == 31 else ""),
                     dict(B=320, T=192, C=64, K=kt), bf3, dgsum=kt == 31))
    cs.append(_c("dw_bwd_grid", "glu_dwconv_bwd", "glu_dwconv_bwd EINVAL(grid.y)", dict(B=65536, T=1, C=1, K=1)))
    return cs


def _apb_cases():
    cs = []
    for op in ("add_pos_bias", "add_pos_bias_bwd"):
        cs.append(_c(op + "_vec", op, op + "_bf16 vec", dict(M=203, d=72), dict(x="bf16")))
        cs.append(_c(op + "_f32", op, op + " generic(f32)", dict(M=203, d=72)))
        cs.append(_c(op + "_bf16_d", op, op + " generic(bf16 d%8)", dict(M=203, d=36), dict(x="bf16")))
        # the smallest M * d over the 4096 x 256 cap with d = 24 (three 16-byte lanes per row) and d = 6
        cs.append(_c(op + "_vec_wrap", op, op + "_bf16 vec wrap", dict(M=349526, d=24), dict(x="bf16")))
        cs.append(_c(op + "_f32_wrap", op, op + " generic(f32) wrap", dict(M=174763, d=6)))
    return cs


def _sm_cases():
    cs = []
    bf = dict(s="bf16", p="bf16", dp="bf16", o="bf16")
    three = ("none", "tail", "all")
    for nv, T, B, H in ((2, 37, 3, 2), (4, 200, 3, 1), (8, 300, 1, 2), (18, 1120, 1, 1), (32, 1160, 1, 1), (0, 2056, 1, 1)):
        masks = three if B == 3 else ("tail",)
        rows = " rows%4" if (B * H * T) % 4 else ""
        cs.append(_c(f"sm_fwd_nv{nv}", "relpos_softmax_fwd", f"relpos_softmax_fwd<NV={nv}>{rows} keymask({','.join(masks)})",
                     dict(B=B, H=H, T=T), masks=masks))
        cs.append(_c(f"sm_bwd_nv{nv}", "relpos_softmax_bwd", f"relpos_softmax_bwd<NV={nv}>", dict(B=B, H=H, T=T)))
    cs.append(_c("sm_fwd_nv2_ragged", "relpos_softmax_fwd", "relpos_softmax_fwd<NV=2> ragged", dict(B=5, H=2, T=70), ragged=True,
                 lens=RAGGED_LENS_70))
    cs.append(_c("sm_fwd_nv18_ragged", "relpos_softmax_fwd", "relpos_softmax_fwd<NV=18> ragged", dict(B=5, H=1, T=520), ragged=True,
                 lens=(0, 1, 520, 64, 65)))
    cs.append(_c("sm_fwd_bf16_gen", "relpos_softmax_fwd", "relpos_softmax_fwd<NV=2> bf16 rows%4 keymask(none,tail,all)",
                 dict(B=3, H=1, T=37), bf, masks=three))
    cs.append(_c("sm_bwd_bf16_gen", "relpos_softmax_bwd", "relpos_softmax_bwd<NV=2> bf16", dict(B=3, H=1, T=37), bf))
    for nc, T, B, H in ((1, 72, 3, 2), (2, 520, 1, 2), (3, 1032, 1, 1), (4, 1544, 1, 1)):
        masks = three if B == 3 else ("tail",)
        cs.append(_c(f"sm_fwd_nc{nc}", "relpos_softmax_fwd", f"relpos_softmax_fwd_bf16<NC={nc}> keymask({','.join(masks)})",
                     dict(B=B, H=H, T=T), bf, masks=masks))
        cs.append(_c(f"sm_bwd_nc{nc}", "relpos_softmax_bwd", f"relpos_softmax_bwd_bf16<NC={nc}>", dict(B=B, H=H, T=T), bf))
    cs.append(_c("sm_fwd_drop", "relpos_softmax_fwd", "relpos_softmax_fwd<NV=4> keymask(none,tail,all) drop", dict(B=3, H=2, T=200),
                 masks=three, drop_p=0.1, drop_key=777))
    cs.append(_c("sm_fwd_drop_bf16", "relpos_softmax_fwd", "relpos_softmax_fwd_bf16<NC=1> keymask(none,tail,all) drop", dict(B=3, H=2, T=200),
                 bf, masks=three, drop_p=0.1, drop_key=4242))
    cs.append(_c("sm_bwd_head_major", "relpos_softmax_bwd", "relpos_softmax_bwd_bf16<NC=1> head_major", dict(B=3, H=2, T=72), bf,
                 head_major=True))
    cs.append(_c("sm_bwd_head_major_gen", "relpos_softmax_bwd", "relpos_softmax_bwd<NV=2> head_major", dict(B=3, H=2, T=37), head_major=True))
    cs.append(_c("sm_bwd_inplace", "relpos_softmax_bwd", "relpos_softmax_bwd<NV=4> inplace", dict(B=2, H=2, T=200), inplace=True))
    cs.append(_c("sm_bwd_inplace_nv0", "relpos_softmax_bwd", "relpos_softmax_bwd<NV=0> inplace", dict(B=1, H=1, T=2056), inplace=True))
    cs.append(_c("sm_bwd_rowscale", "relpos_softmax_bwd", "relpos_softmax_bwd_bf16<NC=1> rowscale", dict(B=2, H=2, T=200), bf, rowscale=True))
    cs.append(_c("sm_bwd_rowscale_gen", "relpos_softmax_bwd", "relpos_softmax_bwd EINVAL(rowscale on generic)", dict(B=2, H=2, T=37),
                 rowscale=True))
    cs.append(_c("sm_bwd_drop_stored", "relpos_softmax_bwd", "relpos_softmax_bwd_bf16<NC=1> drop(stored)", dict(B=3, H=2, T=200), bf,
                 drop_p=0.1, drop_key=4242, stored_mask=True))
    cs.append(_c("sm_bwd_drop_regen", "relpos_softmax_bwd", "relpos_softmax_bwd_bf16<NC=1> drop(regen)", dict(B=3, H=2, T=200), bf,
                 drop_p=0.1, drop_key=4242))
    cs.append(_c("sm_bwd_drop_stored_gen", "relpos_softmax_bwd", "relpos_softmax_bwd<NV=4> drop(stored)", dict(B=3, H=2, T=200),
                 drop_p=0.1, drop_key=777, stored_mask=True))
    cs.append(_c("sm_bwd_drop_regen_gen", "relpos_softmax_bwd", "relpos_softmax_bwd EINVAL(regenerated mask on generic)",
                 dict(B=1, H=1, T=37), drop_p=0.1, drop_key=777))
    return cs


CASES = _ln_cases() + _col_bn_cases() + _dw_cases() + _apb_cases() + _sm_cases()
for _case in CASES:
    _lab, _facts = expected_path(_case["op"], _case["shape"], _case["dtypes"], _case["aligned"], _case["options"])
    _case["predicted"], _case["facts"] = _lab, _facts
    _case["L"] = case_L(_case) if _facts["rc"] == 0 else None
CASE_BY_ID = {c["id"]: c for c in CASES}


def _required():
    r = []
    for nq in (1, 2, 3, 4):
        r += [f"ln_fwd_vec<NQ={nq}>", f"ln_fwd_vec<NQ={nq}> ragged"]
    for v in (1, 2, 4, 6, 8, 24):
        r += [f"ln_fwd<V={v}>", f"ln_fwd<V={v}> ragged"]
    r += ["ln_fwd_vec<NQ=3> y16", "ln_fwd<V=6> y16", "ln_fwd<V=6> misaligned"]
    for np_ in (1, 2, 3, 4):
        r += [f"ln_bwd_row64<NP={np_}> dxsum", f"ln_bwd_row64<NP={np_},DY16> dxsum"]
    r += ["ln_bwd_row64<NP=3> pipeline dxsum", "ln_bwd_row64<NP=3,DY16> pipeline dx16 dxsum", "ln_bwd_row64<NP=1> pipeline dxsum",
          "ln_bwd_row64<NP=3> short-block dxsum", "ln_bwd_row64<NP=3> no-dres", "ln_bwd_row64<NP=3> dx16 dxsum drop",
          "ln_bwd_row64<NP=3,DY16> pipeline dx16 dxsum drop"]
    for v in (1, 2, 4, 6, 8, 24):
        r += [f"ln_bwd<V={v}> dx16 dxsum", f"ln_bwd<V={v}> dy16 dx16 dxsum"]
    r += ["ln_bwd<V=1> wrap dxsum", "ln_bwd<V=6> dxsum", "ln_bwd EINVAL(drop on generic)"]
    r += ["col_reduce_vec mode=0", "col_reduce_vec mode=1 M<16", "col_reduce_vec mode=2 blocks>1",
          "col_reduce generic(bf16 x) mode=0 blocks>1", "col_reduce generic(rowmask) mode=1 blocks>1", "col_reduce generic(C%64) mode=2",
          "col_reduce generic(ld%4) mode=2", "col_reduce generic(misaligned) mode=1 M<16", "f64_to_f32_add"]
    r += ["bn_act_fwd vec f32 none train", "bn_act_fwd vec f32 swish train", "bn_act_fwd vec f32 tanh train",
          "bn_act_fwd vec f32 swish eval", "bn_act_fwd vec y16 swish train", "bn_act_fwd vec y16 tanh eval",
          "bn_act_fwd generic f32 swish train", "bn_act_fwd generic f32 tanh eval", "bn_act_fwd generic y16 none train",
          "bn_act_fwd generic y16 swish eval", "bn_act_fwd generic f32 none eval", "bn_act_fwd vec f32 swish train M=2",
          "bn_act_fwd vec f32 swish train wrap", "bn_act_fwd generic f32 swish train wrap"]
    r += ["bn_act_bwd_a vec swish", "bn_act_bwd_a vec tanh", "bn_act_bwd_a generic(C%64) swish", "bn_act_bwd_a generic(dy16) none",
          "bn_act_bwd_b vec swish train", "bn_act_bwd_b vec tanh eval", "bn_act_bwd_b generic(C%4) swish train",
          "bn_act_bwd_b generic(dy16) none train", "bn_act_bwd_b vec swish train wrap", "bn_act_bwd_b generic(C%4) swish train wrap"]
    for kt in (7, 15, 31):
        for kk in ("K==KT", "K<KT"):
            r += [f"glu_dwconv_fwd<KT={kt}> {kk}", f"glu_dwconv_fwd<KT={kt}> {kk} ragged", f"glu_dwconv_fwd_vec<KT={kt}> {kk}"]
        r += [f"glu_dwconv_bwd<KT={kt}> K==KT dgsum", f"glu_dwconv_bwd_vec<KT={kt}> K==KT dgsum"]
    r += ["glu_dwconv_fwd<KT=15> K==KT bf16", "glu_dwconv_fwd<KT=31> K==KT T=1", "glu_dwconv_fwd_vec<KT=31> K==KT T=pad",
          "glu_dwconv_fwd<KT=7> K==KT T=63", "glu_dwconv_fwd_vec<KT=15> K==KT T=64", "glu_dwconv_fwd<KT=31> K==KT T=65",
          "glu_dwconv_fwd EINVAL(grid.y)", "glu_dwconv_bwd<KT=15> K<KT", "glu_dwconv_bwd_vec<KT=31> K<KT",
          "glu_dwconv_bwd<KT=7> K==KT bf16 dgsum", "glu_dwconv_bwd<KT=7> K==KT tpb>1 dgsum", "glu_dwconv_bwd<KT=31> K==KT tpb>1",
          "glu_dwconv_bwd_vec<KT=7> K==KT tpb>1", "glu_dwconv_bwd_vec<KT=31> K==KT tpb>1 dgsum", "glu_dwconv_bwd EINVAL(grid.y)"]
    for op in ("add_pos_bias", "add_pos_bias_bwd"):
        r += [op + "_bf16 vec", op + " generic(f32)", op + " generic(bf16 d%8)", op + "_bf16 vec wrap", op + " generic(f32) wrap"]
    r += ["relpos_softmax_fwd<NV=2> rows%4 keymask(none,tail,all)", "relpos_softmax_fwd<NV=4> keymask(none,tail,all)",
          "relpos_softmax_fwd<NV=8> keymask(tail)", "relpos_softmax_fwd<NV=18> keymask(tail)", "relpos_softmax_fwd<NV=32> keymask(tail)",
          "relpos_softmax_fwd<NV=0> keymask(tail)", "relpos_softmax_fwd<NV=2> ragged", "relpos_softmax_fwd<NV=18> ragged",
          "relpos_softmax_fwd<NV=2> bf16 rows%4 keymask(none,tail,all)", "relpos_softmax_fwd_bf16<NC=1> keymask(none,tail,all)",
          "relpos_softmax_fwd_bf16<NC=2> keymask(tail)", "relpos_softmax_fwd_bf16<NC=3> keymask(tail)",
          "relpos_softmax_fwd_bf16<NC=4> keymask(tail)", "relpos_softmax_fwd<NV=4> keymask(none,tail,all) drop",
          "relpos_softmax_fwd_bf16<NC=1> keymask(none,tail,all) drop"]
    r += [f"relpos_softmax_bwd<NV={nv}>" for nv in (2, 4, 8, 18, 32, 0)] + [f"relpos_softmax_bwd_bf16<NC={nc}>" for nc in (1, 2, 3, 4)]
    r += ["relpos_softmax_bwd<NV=2> bf16", "relpos_softmax_bwd_bf16<NC=1> head_major", "relpos_softmax_bwd<NV=2> head_major",
          "relpos_softmax_bwd<NV=4> inplace", "relpos_softmax_bwd<NV=0> inplace", "relpos_softmax_bwd_bf16<NC=1> rowscale",
          "relpos_softmax_bwd EINVAL(rowscale on generic)", "relpos_softmax_bwd_bf16<NC=1> drop(stored)",
          "relpos_softmax_bwd_bf16<NC=1> drop(regen)", "relpos_softmax_bwd<NV=4> drop(stored)",
          "relpos_softmax_bwd EINVAL(regenerated mask on generic)"]
    return r


REQUIRED_LABELS = _required()


# ----------------------------------------------------------------------------------------------------------------------
# operands of a case (CPU tensors in the storage types the kernel receives) and its reference
# ----------------------------------------------------------------------------------------------------------------------
def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case["id"].encode()))


def _rn(gen, *shape, scale=1.0, bf=False):
    t = torch.randn(*shape, generator=gen) * scale
    return t.to(torch.bfloat16) if bf else t


def _keymask(masks, B, T, gen):
    m = torch.ones(B, T, dtype=torch.uint8)
    for b in range(B):
        kind = masks[b % len(masks)]
        if kind == "tail":
            m[b, int(torch.randint(1, T, (1,), generator=gen)):] = 0
        elif kind == "all":
            m[b] = 0
    return m


def make_inputs(case):
    """The operands of a case, deterministic in its id."""
    op, s, dt, o, gen = case["op"], case["shape"], case["dtypes"], case["options"], _gen(case)
    bf = lambda k: dt.get(k, "f32") == "bf16"      # noqa: E731
    if op == "ln_fwd":
        M, D = s["M"], s["D"]
        x = _rn(gen, M, D) + 0.5
        inp = dict(x=x, g=1 + 0.2 * _rn(gen, D), b=0.1 * _rn(gen, D), eps=1e-5 if D % 2 else 1e-12)
        if o.get("ragged"):
            B, T = o["B"], o["T"]
            for b, n in enumerate(o["lens"]):      # what lies behind a row's length must not be read
                x[b * T + n:(b + 1) * T] = float("nan")
            inp["lens"] = torch.tensor(o["lens"], dtype=torch.int32)
        return inp
    if op == "ln_bwd":
        M, D = s["M"], s["D"]
        x = _rn(gen, M, D) + 0.5
        r = ref_layernorm_fwd(x, torch.ones(D), torch.zeros(D), 1e-5)
        return dict(dy=_rn(gen, M, D, bf=bf("dy")), x=x, g=1 + 0.2 * _rn(gen, D), mean=r["mean"].ref.float(), rstd=r["rstd"].ref.float(),
                    dres=_rn(gen, M, D) if o.get("dres", True) else None)
    if op == "col_reduce":
        M, C, ld = s["M"], s["C"], s.get("ld", s["C"])
        if o.get("ints"):
            x, y = (torch.randint(-8, 9, (M, ld), generator=gen).float() for _ in range(2))
            x = x.to(torch.bfloat16) if bf("x") else x
        else:
            x, y = _rn(gen, M, ld, bf=bf("x")) + 0.25, _rn(gen, M, ld)
        mask = (torch.rand(M, generator=gen) < 0.7).to(torch.uint8) if o.get("rowmask") else None
        return dict(x=x, y=y if o.get("mode", 0) == 2 else None, rowmask=mask)
    if op == "f64_to_f32_add":
        return dict(src=torch.randn(s["n"], generator=gen, dtype=F64), dst=_rn(gen, s["n"]), scale=0.37)
    if op in ("bn_act_fwd", "bn_act_bwd_a", "bn_act_bwd_b"):
        M, C = s["M"], s["C"]
        z = _rn(gen, M, C) * (1 + torch.arange(C) % 3) + 0.3
        g, b = 1 + 0.2 * _rn(gen, C), 0.1 * _rn(gen, C)
        zd = z.to(F64)
        stats = torch.cat([zd.sum(0), (zd * zd).sum(0)])
        inp = dict(z=z, g=g, b=b, stats=stats, rmean=0.1 * _rn(gen, C), rvar=1 + 0.1 * torch.rand(C, generator=gen), eps=1e-5,
                   momentum=0.1)
        if op != "bn_act_fwd":
            mu = zd.mean(0)
            var = (zd * zd).mean(0) - mu * mu
            inp.update(mean=mu.float(), rstd=(1.0 / torch.sqrt(var + 1e-5)).float(), dy=_rn(gen, M, C, bf=bf("dy")))
            if op == "bn_act_bwd_b":
                r = ref_bn_act_bwd_a(inp["dy"], z, inp["mean"], inp["rstd"], g, b, o.get("act", ACT_NONE))
                inp.update(sums=r["sums"].ref, dgamma0=_rn(gen, C), dbeta0=_rn(gen, C))
        return inp
    if op in ("glu_dwconv_fwd", "glu_dwconv_bwd"):
        B, T, C, K = s["B"], s["T"], s["C"], s["K"]
        g = _rn(gen, B * T, 2 * C, bf=bf("g"))
        inp = dict(g=g, w=_rn(gen, C, K, scale=K ** -0.5), bias=_rn(gen, C))
        if o.get("ragged"):
            for b, n in enumerate(o["lens"]):
                g[b * T + n:(b + 1) * T] = float("nan")
            inp["lens"] = torch.tensor(o["lens"], dtype=torch.int32)
        if op == "glu_dwconv_bwd":
            glu = ref_glu_dwconv_fwd(g, inp["w"], inp["bias"], B, T)["glu"].ref
            inp.update(glu=glu.float().to(torch.bfloat16) if bf("glu") else glu.float(), dz=_rn(gen, B * T, C))
        return inp
    if op == "add_pos_bias":
        M, d = s["M"], s["d"]
        return dict(qkv=_rn(gen, M, 3 * d, bf=bf("x")), u=_rn(gen, d), v=_rn(gen, d))
    if op == "add_pos_bias_bwd":
        M, d = s["M"], s["d"]
        return dict(dqu=_rn(gen, M, d, bf=bf("x")), dqv=_rn(gen, M, d, bf=bf("x")))
    if op == "relpos_softmax_fwd":
        B, H, T = s["B"], s["H"], s["T"]
        ac, bd = _rn(gen, B, H, T, T, scale=3.0, bf=bf("s")), _rn(gen, B, H, T, T, scale=3.0, bf=bf("s"))
        inp = dict(ac=ac, bd=bd, scale=0.3)
        if o.get("ragged"):
            for b, n in enumerate(o["lens"]):      # keys and query rows behind the length, and BD outside its [n][n] corner
                ac[b, :, n:, :], ac[b, :, :, n:] = float("nan"), float("nan")
                bd[b, :, n:, :], bd[b, :, :, n:] = float("nan"), float("nan")
            inp["lens"] = torch.tensor(o["lens"], dtype=torch.int32)
        else:
            inp["keymask"] = _keymask(o.get("masks") or ("none",), B, T, gen)
        return inp
    if op == "relpos_softmax_bwd":
        B, H, T = s["B"], s["H"], s["T"]
        km = _keymask(("none", "tail"), B, T, gen)
        pr = ref_relpos_softmax_fwd(_rn(gen, B, H, T, T, scale=3.0), _rn(gen, B, H, T, T, scale=3.0), km, 0.3)["probs"].ref
        inp = dict(dprobs=_rn(gen, B, H, T, T, bf=bf("dp")), scale=0.3, rowscale=None)
        if o.get("rowscale"):          # probs hold un-normalised exponentials, rowscale their normaliser
            rsc = 0.5 + torch.rand(B * H * T, generator=gen)
            pr = pr / rsc.view(B, H, T, 1).to(F64)
            inp["rowscale"] = rsc
        inp["probs"] = pr.float().to(torch.bfloat16) if bf("p") else pr.float()
        inp["dbd0"] = torch.full((B, H, T, T), 7.0, dtype=torch.bfloat16 if bf("o") else torch.float32)
        return inp
    raise KeyError(op)


def reference(case, inp, keep=None):
    """The float64 reference of a case on its operands.  keep: the dropout keep mask read off the kernel's own dropped output."""
    op, s, o = case["op"], case["shape"], case["options"]
    if op == "ln_fwd":
        if o.get("ragged"):
            return ref_layernorm_fwd_ragged(inp["x"], inp["g"], inp["b"], inp["eps"], o["lens"], o["B"], o["T"])
        return ref_layernorm_fwd(inp["x"], inp["g"], inp["b"], inp["eps"])
    if op == "ln_bwd":
        return ref_layernorm_bwd(inp["dy"], inp["x"], inp["g"], inp["mean"], inp["rstd"], inp["dres"], 0.5, keep, o.get("drop_p", 0.0))
    if op == "col_reduce":
        C = s["C"]
        return ref_col_reduce(inp["x"][:, :C], o.get("mode", 0), None if inp["y"] is None else inp["y"][:, :C], inp["rowmask"])
    if op == "f64_to_f32_add":
        a, b = widen(inp["dst"]), inp["src"] * inp["scale"]
        return dict(dst=_out(a + b, a.abs() + b.abs()))
    if op == "bn_act_fwd":
        return ref_bn_act_fwd(inp["z"], inp["stats"], inp["g"], inp["b"], inp["rmean"], inp["rvar"], inp["eps"], inp["momentum"],
                              o.get("training", True), o.get("act", ACT_NONE))
    if op == "bn_act_bwd_a":
        return ref_bn_act_bwd_a(inp["dy"], inp["z"], inp["mean"], inp["rstd"], inp["g"], inp["b"], o.get("act", ACT_NONE))
    if op == "bn_act_bwd_b":
        return ref_bn_act_bwd_b(inp["dy"], inp["z"], inp["mean"], inp["rstd"], inp["g"], inp["b"], inp["sums"], inp["dgamma0"],
                                inp["dbeta0"], o.get("training", True), o.get("act", ACT_NONE))
    if op == "glu_dwconv_fwd":
        if o.get("ragged"):
            return ref_glu_dwconv_fwd_ragged(inp["g"], inp["w"], inp["bias"], o["lens"], s["B"], s["T"])
        return ref_glu_dwconv_fwd(inp["g"], inp["w"], inp["bias"], s["B"], s["T"])
    if op == "glu_dwconv_bwd":
        return ref_glu_dwconv_bwd(inp["dz"], inp["g"], inp["glu"], inp["w"], s["B"], s["T"])
    if op == "add_pos_bias":
        return ref_add_pos_bias(inp["qkv"], inp["u"], inp["v"], s["d"])
    if op == "add_pos_bias_bwd":
        return ref_add_pos_bias_bwd(inp["dqu"], inp["dqv"])
    if op == "relpos_softmax_fwd":
        if o.get("ragged"):
            return ref_relpos_softmax_fwd_ragged(inp["ac"], inp["bd"], o["lens"], inp["scale"])
        return ref_relpos_softmax_fwd(inp["ac"], inp["bd"], inp["keymask"], inp["scale"], keep, o.get("drop_p", 0.0))
    if op == "relpos_softmax_bwd":
        return ref_relpos_softmax_bwd(inp["probs"], inp["dprobs"], inp["scale"], inp["dbd0"], keep, o.get("drop_p", 0.0),
                                      inp["rowscale"], bool(o.get("head_major")))
    raise KeyError(op)


INTRINSIC = {"bn_act_fwd": None, "bn_act_bwd_a": None, "bn_act_bwd_b": None, "glu_dwconv_fwd": "sigmoid", "glu_dwconv_bwd": "sigmoid",
             "relpos_softmax_fwd": "exp"}


def case_intrinsic_error(case, ref):
    """r of the module docstring for a case: 0.0 where no intrinsic is involved."""
    op = case["op"]
    if op not in INTRINSIC or "pre" not in ref:
        return 0.0
    kind = INTRINSIC[op]
    if kind is None:
        act = case["options"].get("act", ACT_NONE)
        if act == ACT_NONE:
            return 0.0
        kind = "sigmoid" if act == ACT_SWISH else "tanh"
    pre = ref["pre"]
    return intrinsic_error(kind, pre[torch.isfinite(pre)])


def keep_rate_interval(n, p, sigmas=5.0):
    """The binomial interval the keep count of n elements at drop probability p (resolution 2^-16) must fall in."""
    q = 1.0 - math.floor(p * 65536.0) / 65536.0
    sd = math.sqrt(n * q * (1.0 - q))
    return n * q - sigmas * sd, n * q + sigmas * sd
