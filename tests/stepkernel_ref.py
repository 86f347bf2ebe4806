"""References, launch geometry and the case table for the step kernels of csrc/misc.hip: the counter-based dropout generator
(csrc/dtype_io.h), the masked L1/L2 loss, the gradient norm and clip+Adam on the flat buffers, the encoder prologue and the
element-wise helpers.  Used by tests/test_stepkernel_ref_host.py (no GPU) and tests/test_gpu_stepkernels.py.

Parts
* `rng_pair` / `keep` / `keep_mask`: the generator in numpy uint32, restated from dtype_io.h.
* `*_exact`: operations whose every output bit is fixed by the kernel text (copies, casts, one- and two-rounding element-wise
  arithmetic; the library is built with -ffp-contract=off, so a * x + y is two roundings).  They return numpy fp32 arrays or torch
  bf16 tensors and are compared bit for bit (NaN by isnan).
* `*_ref`: float64 references of the accumulating operations.  They return `Approx(ref, mag, L, r)`.
* `geometry(op, sizes, aligned)`: the grid, the trips of the grid-stride loop, the body (16-byte or scalar), the tail and the label
  of one call, derived from the launchers: nblocks(n, cap) = clamp(ceil(n / 256), 1, cap) with cap 4096 (8192 for the casts, 2048
  for the Adam sweep, 64 for splice_spans), LOSS_BLOCKS = 512, SUMSQ_BLOCKS = 1024, 128 rows per block of dropout_bwd_cast.
* `CASES`: the smallest shapes that reach each label; `REQUIRED_LABELS` is the contract, the set the table reaches must equal it.

Bounds.  An fp32 rounding has relative error at most u = 2^-24.  With L roundings on the longest path to an output and `mag` the
same formula with every term replaced by its absolute value, the first-order error is L u mag; the bound used is

    |got - ref| <= (L 2^-23 + 2 r) mag,

twice the first-order term, which covers the higher orders while L 2^-24 << 1.  r is non-zero only for bias_act TANH, where it is
rowkernel_ref.intrinsic_error("tanh", pre), doubled as in that file.  A bf16 output is compared bit for bit against the rounding of
the exactly restated fp32 value.  L per output (read off the kernels):

* sumsq norm.  A lane squares (1 rounding) and adds A values in fp32 between two folds into double: relative error of the sum of
  squares (A + 1) u, halved by the square root, then (float) and * |gscale|: L = ceil((A + 1) / 2) + 2.  A = min(32, vector trips)
  (+ 1 for the lane that also takes a tail element) on the 16-byte path -- the fold happens when a lane's count reaches 32 -- and
  ceil(n / 262144) on the scalar path, which adds everything into f0 and folds once.
* loss.  Per element x - y (1) and the square (1; fabsf is exact); a lane adds 2 ceil(C / 64) terms per row (before and after) for
  `rows per wave` rows, 6 more additions in the xor tree and 3 across the waves; the block partials are summed in double; then
  (float) (1), inv = 1 / (n + 1e-10f) (2) and the product (1): L = 2 ceil(C / 64) rows_per_wave + 6 + 3 + 6.  Every term is
  non-negative, so mag is the loss itself, sum |d|^(1 or 2) / n.  The gradients are restated bit for bit.
* Adam.  Lc = roundings of coef: 0 when coef = 1 * gscale exactly (clip <= 0, or clip / (norm + 1e-6) > 1), else L_norm + 3
  (+ 1e-6f, the division, * gscale).  gi = g coef: Lc + 1.  m' = m b1 + (1 - b1) gi (1 - b1 is exact for b1 in [0.5, 1], Sterbenz):
  L_m = Lc + 3, mag_m = |m b1| + |(1 - b1) gi|.  v' = v b2 + ((1 - b2) gi) gi: L_v = 2 (Lc + 1) + 3, mag_v = v'.
  denom = sqrt(v') / bc2s + eps: L_v / 2 for v', the root, bc2s (rounded once from double), the division, + eps:
  L_den = ceil(L_v / 2) + 4.  step_size = lr / bc1: lr (noam: rounded once from double; host entry: given as fp32, 0), bc1 (1), the
  division (1).  p' = p - step_size m' / denom: L_p = L_m + L_den + L_step + 3 (product, quotient, difference) with
  mag_p = |p| + step_size mag_m / denom.
* segment_colsum: a lane adds ceil(T / 4) rows, 3 additions across the four row groups, 1 into the output: L = ceil(T / 4) + 4.
* dropout_bwd_cast colsum: g inv (1), ceil(rows in block / 4) additions, 3 across the row groups, * colsum_scale (1) and one atomic
  addition per row block: L = ceil(min(M, 128) / 4) + 5 + row blocks.
* attn_bias_fold: S additions and at most 2 into the output (d b_q takes the u and the v sum): L = S + 2.
* embed_finish_bwd demb / dseg: one atomic addition per contribution, 2 roundings in the addend: L = contributions + 2.
"""
import collections
import math
import zlib

import numpy as np
import torch

import rowkernel_ref as RK

U23 = 2.0 ** -23
F32 = np.float32
EINVAL = -22
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
LOSS_BLOCKS, SUMSQ_BLOCKS, ADAM_CAP, RPB = 512, 1024, 2048, 128

Approx = collections.namedtuple("Approx", "ref mag L r")


def _cdiv(a, b):
    return -(-a // b)


def bound(o):
    """The tolerance of an Approx output: see the module docstring."""
    return (o.L * U23 + 2.0 * o.r) * np.asarray(o.mag, dtype=np.float64)


def bf16(x):
    """fp32 numpy array -> torch bf16 tensor (round to nearest even)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16)


def widen(t):
    """torch bf16 / numpy fp32 -> numpy fp32 (exact)."""
    return t.to(torch.float32).numpy() if torch.is_tensor(t) else np.asarray(t, dtype=F32)


# ----------------------------------------------------------------------------------------------------------------------
# a. the dropout generator (dtype_io.h)
# ----------------------------------------------------------------------------------------------------------------------
def rng_pair(key, pair):
    """One 32-bit hash per (even, odd) element pair: the RXS-M-XS permutation of (pair ^ key) * 747796405 + (key | 1)."""
    key = np.uint32(int(key) & 0xffffffff)
    pair = np.atleast_1d(np.asarray(pair, dtype=np.uint32))
    state = (pair ^ key) * np.uint32(747796405) + np.full(1, key | np.uint32(1), dtype=np.uint32)
    word = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
    return (word >> np.uint32(22)) ^ word


def thr16(p):
    """(unsigned int)((double)(float)p * 2^32) >> 16: the 16-bit threshold an element's bits are compared with."""
    return (int(float(F32(p)) * 4294967296.0) & 0xffffffff) >> 16


def drop_inv(p):
    return F32(1) / (F32(1) - F32(p))


def keep(key, idx, p):
    """Keep flags of the elements idx (any integers, taken modulo 2^32): even indices take the low 16 bits of the pair's hash,
    odd indices the high 16 bits; kept when bits >= thr16(p)."""
    idx = np.atleast_1d(np.asarray(idx, dtype=np.int64) & 0xffffffff).astype(np.uint32)
    h = rng_pair(key, idx >> np.uint32(1))
    bits = np.where((idx & np.uint32(1)) != 0, h >> np.uint32(16), h & np.uint32(0xffff))
    return bits >= np.uint32(thr16(p))


def keep_mask(key, n, p, first=0):
    return keep(key, first + np.arange(n, dtype=np.int64), p)


def keep_rate(p):
    return 1.0 - math.floor(float(F32(p)) * 65536.0) / 65536.0


# ----------------------------------------------------------------------------------------------------------------------
# b. the masked loss
# ----------------------------------------------------------------------------------------------------------------------
def mlm_loss_ref(before, after, target, masked, l2, gscale, want=(True, True)):
    """float64 loss and magnitude, bit-exact fp32 gradients.  want = (d_before given, d_after given): the launcher writes
    gradients only when d_before is there and (d_after is there or there is no `after`)."""
    rows = np.asarray(masked) != 0
    n = int(rows.sum())
    x, y = before[rows].astype(np.float64), target[rows].astype(np.float64)
    terms = [x - y] + ([after[rows].astype(np.float64) - y] if after is not None else [])
    tot = sum(float((d * d).sum() if l2 else np.abs(d).sum()) for d in terms)
    loss = tot / (n + 1e-10)
    out = dict(loss=loss, mag=loss, n=n, d_before=None, d_after=None)
    if not (want[0] and (want[1] or after is None)):
        return out
    inv = F32(1) / (F32(n) + F32(1e-10))
    k = F32(inv * F32(gscale))

    def grad(a):
        with np.errstate(invalid="ignore"):
            d = (a - target).astype(F32)
            g = (F32(2) * d) * k if l2 else np.where(d > 0, k, np.where(d < 0, -k, F32(0)))
        return np.where(rows[:, None], g, F32(0)).astype(F32)

    out["d_before"] = grad(before)
    if want[1]:
        out["d_after"] = grad(after) if after is not None else np.zeros_like(before)
    return out


def loss_L(M, C):
    g = geometry("loss", dict(M=M, C=C))
    return 2 * g["lane_trips"] * g["rows_per_wave"] + 6 + 3 + 6


def loss_fp32(before, after, target, masked, l2):
    """The loss evaluated in fp32 in the kernel's order (lane sums over rows and 64-column trips, xor tree, four waves, blocks in
    double, float(sum) * inv)."""
    M, C = before.shape
    nblk = min(_cdiv(M, 4), LOSS_BLOCKS)
    W = nblk * 4
    lanes, cnt = np.zeros((W, 64), F32), np.zeros(W, F32)
    for r0 in range(0, M, W):
        rows = np.arange(r0, min(M, r0 + W))
        sel = masked[rows] != 0
        cnt[:len(rows)] += sel.astype(F32)
        for c0 in range(0, C, 64):
            cols = np.arange(c0, min(C, c0 + 64))
            y = target[np.ix_(rows, cols)]
            for a in ([before, after] if after is not None else [before]):
                with np.errstate(invalid="ignore"):
                    d = (a[np.ix_(rows, cols)] - y).astype(F32)
                    t = (d * d).astype(F32) if l2 else np.abs(d)
                lanes[:len(rows), :len(cols)] += np.where(sel[:, None], t, F32(0))
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, idx ^ o]).astype(F32)
    s = lanes[:, 0].reshape(nblk, 4)
    c = cnt.reshape(nblk, 4)
    bs = ((s[:, 0] + s[:, 1]).astype(F32) + s[:, 2]).astype(F32) + s[:, 3]
    bc = ((c[:, 0] + c[:, 1]).astype(F32) + c[:, 2]).astype(F32) + c[:, 3]
    n = F32(bc.astype(np.float64).sum())
    inv = F32(1) / (n + F32(1e-10))
    return float(F32(bs.astype(np.float64).sum()) * inv)


# ----------------------------------------------------------------------------------------------------------------------
# c. gradient norm and Adam
# ----------------------------------------------------------------------------------------------------------------------
def sumsq_ref(g):
    g = np.asarray(g, dtype=np.float64)
    return float((g * g).sum())


def norm_L(n, aligned):
    return _cdiv(geometry("sumsq", dict(n=n), aligned)["adds"] + 1, 2) + 2


def sumsq_fp32(g, aligned):
    """sum g^2 with the kernel's lane sums: four fp32 partials per lane over 16-byte vectors, folded into double every 32 vectors,
    the tail (everything, when g is not 16-byte aligned) into the first partial."""
    n, nthr = g.size, SUMSQ_BLOCKS * 256
    n4 = n // 4 if aligned else 0
    s, f = np.zeros(nthr, np.float64), np.zeros((nthr, 4), F32)
    sq = (g[:n4 * 4] * g[:n4 * 4]).astype(F32).reshape(n4, 4)
    for t in range(_cdiv(n4, nthr)):
        ch = sq[t * nthr:(t + 1) * nthr]
        f[:len(ch)] += ch
        if (t + 1) % 32 == 0:
            s[:len(ch)] += f[:len(ch)].astype(np.float64).sum(1)
            f[:len(ch)] = 0
    tail = (g[n4 * 4:] * g[n4 * 4:]).astype(F32)
    for t in range(_cdiv(tail.size, nthr)):
        ch = tail[t * nthr:(t + 1) * nthr]
        f[:len(ch), 0] += ch
    return float((s + f.astype(np.float64).sum(1)).sum())


def noam_lr64(t, base_lr, model_size, warmup):
    return float(F32(base_lr)) * float(F32(model_size)) ** -0.5 * min(t ** -0.5, t * float(F32(warmup)) ** -1.5)


def adam_ref(p, g, m, v, t, lr, clip, gscale, betas=(0.9, 0.999), eps=1e-8, aligned=True):
    """float64 clip + Adam step t on the fp32 inputs and float32(beta).  lr: a float (the host entry point; taken as fp32) or
    (base_lr, model_size, warmup) (the Noam entry point).  Returns p, m, v as Approx, the norm as Approx, `skip` and the clock
    increment.  A non-finite norm changes nothing."""
    n = p.size
    p64, g64, m64, v64 = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    with np.errstate(over="ignore", invalid="ignore"):
        norm = math.sqrt(float((g64 * g64).sum())) * abs(float(F32(gscale))) if np.isfinite(g64).all() else float("nan")
    Ln = norm_L(n, aligned)
    out = dict(norm=Approx(norm, abs(norm), Ln, 0.0), skip=not math.isfinite(norm))
    if out["skip"]:
        return out
    b1, b2, e, gs = (float(F32(x)) for x in (betas[0], betas[1], eps, gscale))
    noam = isinstance(lr, tuple)
    lr64 = noam_lr64(t, *lr) if noam else float(F32(lr))
    raw = float(F32(clip)) / (norm + 1e-6) if clip > 0 else 1.0
    out["clip_margin"] = abs(raw - 1.0) if clip > 0 else 1.0
    Lc = Ln + 3 if (clip > 0 and raw < 1.0) else 0
    coef = min(raw, 1.0) * gs
    gi = g64 * coef
    mm = np.abs(m64 * b1) + np.abs((1 - b1) * gi)
    m1 = m64 * b1 + (1 - b1) * gi
    v1 = v64 * b2 + (1 - b2) * gi * gi
    bc1, bc2s = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
    step = lr64 / bc1
    den = np.sqrt(v1) / bc2s + e
    p1 = p64 - step * m1 / den
    L_m, L_v = Lc + 3, 2 * (Lc + 1) + 3
    L_p = L_m + (_cdiv(L_v, 2) + 4) + (3 if noam else 2) + 3
    out.update(p=Approx(p1, np.abs(p64) + step * mm / den, L_p, 0.0), m=Approx(m1, mm, L_m, 0.0), v=Approx(v1, v1, L_v, 0.0),
               lr=lr64, bc1=bc1, bc2s=bc2s)
    return out


def adam_fp32(p, g, m, v, t, lr, clip, gscale, betas=(0.9, 0.999), eps=1e-8, aligned=True, host_powf=False):
    """The kernels' arithmetic in numpy fp32 (norm from sumsq_fp32).  host_powf: bc1 / bc2s as a3t_clip_adam computed them before
    this file existed, 1.f - powf(beta, t) in float."""
    b1, b2, e, gs, cl = F32(betas[0]), F32(betas[1]), F32(eps), F32(gscale), F32(clip)
    norm = F32(F32(math.sqrt(sumsq_fp32(g, aligned))) * abs(gs))
    if isinstance(lr, tuple):
        lr32 = F32(noam_lr64(t, *lr))
    else:
        lr32 = F32(lr)
    if host_powf:
        bc1 = F32(1) - F32(np.power(b1, F32(t)))
        bc2s = np.sqrt(F32(1) - F32(np.power(b2, F32(t))))
    else:
        bc1, bc2s = F32(1.0 - float(b1) ** t), F32(math.sqrt(1.0 - float(b2) ** t))
    coef = cl / (norm + F32(1e-6)) if cl > 0 else F32(1)
    coef = F32((F32(1) if coef > 1 else coef) * gs)
    step = F32(lr32 / bc1)
    gi = (g * coef).astype(F32)
    m1 = ((m * b1).astype(F32) + ((F32(1) - b1) * gi).astype(F32)).astype(F32)
    v1 = ((v * b2).astype(F32) + (((F32(1) - b2) * gi).astype(F32) * gi).astype(F32)).astype(F32)
    den = ((np.sqrt(v1).astype(F32) / bc2s).astype(F32) + e).astype(F32)
    p1 = (p - ((step * m1).astype(F32) / den).astype(F32)).astype(F32)
    return dict(p=p1, m=m1, v=v1, norm=float(norm))


# ----------------------------------------------------------------------------------------------------------------------
# d. exact restatements and the references of the small accumulating kernels
# ----------------------------------------------------------------------------------------------------------------------
def store(x, kind):
    return bf16(x) if kind == "bf16" else np.asarray(x, dtype=F32)


def mask_fill_exact(x, masked, mf, kind="f32"):
    return store(np.where((masked != 0)[:, None], mf[None, :], x), kind)


def scale_exact(x, s):
    return (x * F32(s)).astype(F32)


def axpy_exact(x, y, a):
    return (y + (F32(a) * x).astype(F32)).astype(F32)


def slice_rows_exact(x, B, T, Tm, D, kind="f32"):
    return store(x.reshape(B, T, D)[:, :Tm].reshape(B * Tm, D), kind)


def slice_rows_reverse_exact(x, y, B, T, Tm, D):
    out = x.reshape(B, T, D).copy()
    out[:, :Tm] = (out[:, :Tm] + widen(y).reshape(B, Tm, D)).astype(F32)
    return out.reshape(B * T, D)


def split_bf16_exact(x):
    hi = bf16(x)
    with np.errstate(invalid="ignore"):
        lo = bf16((x - widen(hi)).astype(F32))
    return hi, lo


def cast_conv_t_exact(W):
    """Wt[c][taps - 1 - t][n] = bf16(W[n][t][c])."""
    return bf16(W[:, ::-1, :].transpose(2, 1, 0).copy())


def bias_act_ref(x, bias, act, scale):
    """NONE / RELU: the exact fp32 array.  TANH: Approx of the float64 tanh of the fp32 argument."""
    v = (x * F32(scale)).astype(F32)
    if bias is not None:
        v = (v + bias[None, :]).astype(F32)
    if act == ACT_RELU:
        return np.maximum(v, F32(0))
    if act == ACT_TANH:
        t = np.tanh(v.astype(np.float64))
        return Approx(t, np.abs(t), 2, RK.intrinsic_error("tanh", torch.from_numpy(v.astype(np.float64))))
    return v


def segment_colsum_ref(x, out0, B, T):
    x64 = x.astype(np.float64).reshape(B, T, -1)
    return Approx(out0 + x64.sum(1), np.abs(out0) + np.abs(x64).sum(1), _cdiv(T, 4) + 4, 0.0)


def attn_bias_fold_ref(slots, S, d, gu0, gv0, gb0):
    s = slots.astype(np.float64).reshape(S, 4, d)
    a, ma = s.sum(0), np.abs(s).sum(0)
    gb = gb0.astype(np.float64).copy()
    mb = np.abs(gb)
    gb[:d] += a[0] + a[1]
    mb[:d] += ma[0] + ma[1]
    gb[d:] += a[2:].reshape(-1)
    mb[d:] += ma[2:].reshape(-1)
    L = S + 2
    return dict(gu=Approx(gu0 + a[0], np.abs(gu0) + ma[0], L, 0.0), gv=Approx(gv0 + a[1], np.abs(gv0) + ma[1], L, 0.0),
                gbqkv=Approx(gb, mb, L, 0.0))


def dropout_exact(x, p, key, scale=1.0, kind="f32", first=0):
    """y = keep ? fl(fl(x scale) inv) : 0, stored as `kind`; x fp32 numpy or a torch bf16 tensor."""
    x = widen(x).reshape(-1)
    v = ((x * F32(scale)).astype(F32) * drop_inv(p)).astype(F32)
    return store(np.where(keep_mask(key, x.size, p, first), v, F32(0)), kind)


def dropout_bwd_cast_ref(g, p, key, colsum0, colsum_scale, kind="f32"):
    M, C = g.shape
    gm = np.where(keep_mask(key, M * C, p).reshape(M, C), (g * drop_inv(p)).astype(F32), F32(0)).astype(F32)
    out = dict(gm=store(gm, kind))
    if colsum0 is not None:
        cs = float(F32(colsum_scale))
        L = _cdiv(min(M, RPB), 4) + 5 + _cdiv(M, RPB)
        out["colsum"] = Approx(colsum0 + cs * gm.astype(np.float64).sum(0), np.abs(colsum0) + abs(cs) * np.abs(gm).astype(np.float64).sum(0),
                               L, 0.0)
    return out


def embed_finish_fwd_exact(e, emb, seg, text, spos, tpos, B, Tm, Tp, D, xscale, p=0.0, key=0, spk=None):
    """xs[b][t] = dropout(t < Tm ? relu(e[b][t]) xscale : emb[text[b][t - Tm]] xscale) + (seg[pos] + spk[b]); the dropout runs on
    the linear index of xs."""
    xs = F32(xscale)
    sp = (np.maximum(e, F32(0)) * xs).astype(F32).reshape(B, Tm, D)
    tx = (emb[text.reshape(-1)] * xs).astype(F32).reshape(B, Tp, D)
    v = np.concatenate([sp, tx], axis=1)
    if p > 0:
        v = np.where(keep_mask(key, v.size, p).reshape(v.shape), (v * drop_inv(p)).astype(F32), F32(0)).astype(F32)
    sg = np.zeros_like(v)
    if seg is not None:
        sg = np.concatenate([seg[spos.reshape(-1)].reshape(B, Tm, D), seg[tpos.reshape(-1)].reshape(B, Tp, D)], axis=1)
    if spk is not None:
        sg = (sg + spk[:, None, :]).astype(F32)
    return (v + sg).astype(F32).reshape(B * (Tm + Tp), D)


def embed_finish_bwd_ref(dxs, e, text, spos, tpos, B, Tm, Tp, D, V, nseg, xscale, p=0.0, key=0, with_seg=True, demb0=None, dseg0=None):
    """de exact; demb / dseg as Approx on top of demb0 / dseg0.  Rows V - 1 of demb and nseg - 1 of dseg (padding_idx) get
    nothing; dseg takes the gradient in front of the dropout."""
    xs = F32(xscale)
    g = dxs.reshape(B, Tm + Tp, D)
    gd = g
    if p > 0:
        gd = np.where(keep_mask(key, g.size, p).reshape(g.shape), (g * drop_inv(p)).astype(F32), F32(0)).astype(F32)
    de = np.where(e.reshape(B, Tm, D) > 0, (gd[:, :Tm] * xs).astype(F32), F32(0)).astype(F32).reshape(B * Tm, D)
    out = dict(de=de)

    def scatter(base, ids, vals, skip):
        ref = np.zeros_like(base, dtype=np.float64) + base
        mag, cnt = np.abs(ref), np.zeros(base.shape[0], dtype=np.int64)
        ok = ids != skip
        np.add.at(ref, ids[ok], np.asarray(vals[ok], dtype=np.float64))
        np.add.at(mag, ids[ok], np.abs(np.asarray(vals[ok], dtype=np.float64)))
        np.add.at(cnt, ids[ok], 1)
        return Approx(ref, mag, int(cnt.max()) + 2, 0.0)

    # the atomics' addends in float64 from the fp32 constants inv and xscale (their two roundings are in L)
    gd64 = g.astype(np.float64)
    if p > 0:
        gd64 = np.where(keep_mask(key, g.size, p).reshape(g.shape), gd64 * float(drop_inv(p)), 0.0)
    out["demb"] = scatter(demb0, text.reshape(-1), (gd64[:, Tm:] * float(xs)).reshape(B * Tp, D), V - 1)
    if with_seg:
        ids = np.concatenate([spos.reshape(B, Tm), tpos.reshape(B, Tp)], axis=1).reshape(-1)
        out["dseg"] = scatter(dseg0, ids, g.reshape(-1, D), nseg - 1)
    return out


def collate_paint_exact(fs, fe, alen, sel, mspan, nms, flen, tlen, Tm, Tp, sega):
    B, P = fs.shape
    masked, smask, sp = np.zeros((B, Tm), np.uint8), np.zeros((B, Tm), np.uint8), np.zeros((B, Tm), np.int64)
    tmask, tp = np.zeros((B, Tp), np.uint8), np.zeros((B, Tp), np.int64)
    for b in range(B):
        L = min(int(alen[b]), P)
        t = np.arange(Tm)
        m = np.zeros(Tm, bool)
        for j in range(L):                       # later phones overwrite earlier ones
            hit = (t >= fs[b, j]) & (t < fe[b, j])
            sp[b, hit] = j + 1
            if sel[b, j]:
                m |= hit
        for q in range(int(nms[b])):
            m |= (t >= mspan[b, q, 0]) & (t < mspan[b, q, 1])
        valid = t < flen[b]
        masked[b], smask[b] = m & valid, valid
        j = np.arange(Tp)
        tmask[b] = j < tlen[b]
        tp[b] = np.where(j < L, j + 1, 0)
    if not sega:
        sp[:], tp[:] = 0, 0
    return dict(masked=masked, smask=smask, tmask=tmask, sp=sp, tp=tp)


def splice_spans_exact(after, speech, mask, spans, Tout):
    B, Tin, C = speech.shape
    out, lens = np.zeros((B, Tout, C), F32), np.zeros(B, np.int32)
    for b in range(B):
        L = int((mask[b] != 0).sum())
        lens[b] = L
        t = np.arange(min(L, Tin, Tout))
        ins = (t >= spans[b, 0]) & (t < spans[b, 1])
        out[b, :len(t)] = np.where(ins[:, None], after[b, :len(t)], speech[b, :len(t)])
    return out, lens


# ----------------------------------------------------------------------------------------------------------------------
# e. launch geometry
# ----------------------------------------------------------------------------------------------------------------------
def nblocks(n, cap=4096):
    return int(min(cap, max(1, _cdiv(n, 256))))


def _trips(n):
    return "1trip" if n <= 1 else f"{n}trips"


def geometry(op, sizes, aligned=True):
    """What the launcher of `op` does with a call of these sizes: dict(grid, trips, body, tail, label, ...).  `aligned`: every
    pointer the kernel looks at is 16-byte aligned."""
    s = sizes
    if op in ("mask_fill", "scale", "scale_dev", "axpy", "bias_act", "dropout", "slice_rows", "embed_fwd", "embed_bwd", "loss_grad"):
        n = s["n"]
        grid = nblocks(n)
        t = _cdiv(n, grid * 256)
        return dict(grid=grid, trips=t, body="scalar", tail=0, label=f"{op}/{_trips(t)}")
    if op in ("cast_bf16", "split_bf16"):
        n4 = s["n"] // 4
        grid = nblocks(n4, 8192)
        t = _cdiv(n4, grid * 256)
        return dict(grid=grid, trips=t, body="vec", tail=0, label=f"{op}/{'cap/' if grid == 8192 else ''}{_trips(t)}")
    if op == "adam":
        n = s["n"]
        grid = nblocks(n // 4, ADAM_CAP)
        nthr = grid * 256
        n4 = n // 4 if aligned else 0
        tail = n - 4 * n4
        vt, st = _cdiv(n4, nthr), _cdiv(tail, nthr)
        body = ("vec" if n4 else "") + ("+tail" if n4 and tail else "") + ("scalar" if not n4 else "")
        return dict(grid=grid, trips=max(vt, st), vec_trips=vt, tail_trips=st, body=body, tail=tail, label=f"adam/{body}/{_trips(max(vt, st))}")
    if op == "sumsq":
        n, nthr = s["n"], SUMSQ_BLOCKS * 256
        n4 = n // 4 if aligned else 0
        tail = n - 4 * n4
        vt, st = _cdiv(n4, nthr), _cdiv(tail, nthr)
        adds = st if not n4 else min(32, vt) + (1 if tail and vt % 32 else 0)
        adds = max(adds, 1)
        body = ("vec" if n4 else "") + ("+tail" if n4 and tail else "") + ("scalar" if not n4 else "")
        lab = "fold" if vt >= 32 else _trips(max(vt, st))
        return dict(grid=SUMSQ_BLOCKS, trips=max(vt, st), vec_trips=vt, body=body, tail=tail, adds=adds, folds=vt // 32, label=f"sumsq/{body}/{lab}")
    if op == "loss":
        M, C = s["M"], s["C"]
        nblk = min(_cdiv(M, 4), LOSS_BLOCKS)
        rpw, lt = _cdiv(M, nblk * 4), _cdiv(C, 64)
        ctail = "" if C % 64 == 0 else "+ctail"
        return dict(grid=nblk, trips=rpw, rows_per_wave=rpw, lane_trips=lt, body="row", tail=C % 64,
                    label=f"loss/{rpw}row{'s' if rpw > 1 else ''}/{lt}lane{ctail}")
    if op == "dropout_bwd_cast":
        M, C = s["M"], s["C"]
        gx, gy = _cdiv(C, 64), _cdiv(M, RPB)
        return dict(grid=(gx, gy), trips=_cdiv(min(M, RPB), 4), body="col", tail=C % 64, label=f"dropout_bwd_cast/{gx}x{gy}{'+ctail' if C % 64 else ''}")
    if op == "cast_conv_t":
        N, taps, C, count = s["N"], s["taps"], s["C"], s["count"]
        edge = ("+nedge" if N % 32 else "") + ("+cedge" if C % 32 else "")
        return dict(grid=(_cdiv(N, 32) * _cdiv(C, 32), taps, count), trips=1, body="tile", tail=0,
                    label=f"cast_conv_t/{'1tile' if N <= 32 and C <= 32 else 'tiles'}{edge}/{'1tap' if taps == 1 else 'taps'}")
    if op == "segment_colsum":
        return dict(grid=(_cdiv(s["C"], 64), s["B"]), trips=_cdiv(s["T"], 4), body="col", tail=s["C"] % 64,
                    label=f"segment_colsum/{_trips(_cdiv(s['T'], 4))}{'+ctail' if s['C'] % 64 else ''}")
    if op == "attn_bias_fold":
        g = _cdiv(4 * s["d"], 256)
        return dict(grid=g, trips=s["S"], body="col", tail=(4 * s["d"]) % 256, label=f"attn_bias_fold/{'1block' if g == 1 else 'blocks'}")
    if op == "splice_spans":
        m = s["Tout"] * s["C"]
        gx = nblocks(m, 64)
        t = _cdiv(m, gx * 256)
        return dict(grid=(gx, s["B"]), trips=t, count_trips=_cdiv(s["Tin"], 256), body="scalar", tail=0,
                    label=f"splice_spans/{_trips(t)}/count{_cdiv(s['Tin'], 256)}/{'grow' if s['Tout'] > s['Tin'] else 'shrink'}")
    if op == "collate_paint":
        g = _cdiv(max(s["Tm"], s["Tp"]), 256)
        return dict(grid=(g, s["B"]), trips=1, body="scalar", tail=0,
                    label=f"collate_paint/{g}block{'s' if g > 1 else ''}/{'speech' if s['Tm'] >= s['Tp'] else 'text'}")
    raise KeyError(op)


# ----------------------------------------------------------------------------------------------------------------------
# g. the case table
# ----------------------------------------------------------------------------------------------------------------------
def _case(cid, op, label, **kw):
    return dict(id=cid, op=op, label=label, **kw)


def seed_of(cid):
    return zlib.crc32(cid.encode())


def rng_of(cid):
    return np.random.RandomState(seed_of(cid) & 0x7fffffff)


DROP_KEYS = (0, 1, 0xffffffff, 0x9e3779b9, 0x1234abcd)      # the last two stand for "random"
DROP_PS = (0.0, 1e-6, 0.1, 0.5, 0.999)
DROP_NS = (1, 2, 3, 257, (1 << 20) + 259)


def _loss_cases():
    cs = []
    shapes = [(1, 1), (3, 80), (7, 200), (500, 65), (2053, 80)]
    for i, (M, C) in enumerate(shapes):
        lab = geometry("loss", dict(M=M, C=C))["label"]
        # mask / after / l2 / gscale rotate over the shapes, each value with each shape class at least once below
        for j, (mask, after, l2, gs) in enumerate([("all", True, 0, 1.0), ("none", True, 1, 0.5), ("most", False, 1, 1.0), ("most", True, 0, 0.5),
                                                   ("most", False, 0, 1.0), ("most", True, 1, 1.0)]):
            if M == 1 and mask == "most":
                mask = "all"
            cs.append(_case(f"loss_{M}x{C}_{j}", "loss", lab, M=M, C=C, mask=mask, after=after, l2=l2, gscale=gs, want=(True, after)))
    lab = geometry("loss", dict(M=7, C=200))["label"]
    cs.append(_case("loss_only", "loss", lab, M=7, C=200, mask="most", after=True, l2=0, gscale=1.0, want=(False, False)))
    cs.append(_case("loss_after_no_dafter", "loss", lab, M=7, C=200, mask="most", after=True, l2=0, gscale=1.0, want=(True, False)))
    cs.append(_case("loss_nan_unmasked", "loss", geometry("loss", dict(M=500, C=65))["label"], M=500, C=65, mask="most", after=True, l2=1,
                    gscale=0.5, want=(True, True), nan_unmasked=True))
    return cs


def _adam_cases():
    cs = []
    small = (1, 3, 4, 1027)
    for n in small:
        for off in ("none", "all", "g"):
            al = off == "none"       # one float off the 16-byte grid, all four buffers or g alone: the scalar body either way
            gm = geometry("adam", dict(n=n), al)
            cs.append(_case(f"adam_n{n}_off_{off}", "adam", gm["label"], n=n, offset=off, t=7, state="warm", entry="both", clip=1.0, gnorm=0.3,
                            gscale=1.0, aligned=al))
    n2 = (1 << 21) + 1031
    cs.append(_case("adam_2trips", "adam", geometry("adam", dict(n=n2))["label"], n=n2, offset="none", t=7, state="warm", entry="both", clip=1.0,
                    gnorm=5.0, gscale=1.0, aligned=True))
    lab = geometry("adam", dict(n=1027))["label"]
    for t in (1, 2, 3):
        cs.append(_case(f"adam_t{t}_zero", "adam", lab, n=1027, offset="none", t=t, state="zero", entry="both", clip=0.0, gnorm=1.0, gscale=1.0,
                        aligned=True))
    cs.append(_case("adam_t5000_warm", "adam", lab, n=1027, offset="none", t=5000, state="warm", entry="both", clip=1.0, gnorm=0.3, gscale=1.0,
                    aligned=True))
    cs.append(_case("adam_clip_active", "adam", lab, n=1027, offset="none", t=11, state="warm", entry="both", clip=1.0, gnorm=5.0, gscale=1.0,
                    aligned=True))
    cs.append(_case("adam_clip_inactive", "adam", lab, n=1027, offset="none", t=11, state="warm", entry="both", clip=1.0, gnorm=0.3, gscale=1.0,
                    aligned=True))
    cs.append(_case("adam_clip_zero", "adam", lab, n=1027, offset="none", t=11, state="warm", entry="both", clip=0.0, gnorm=5.0, gscale=1.0,
                    aligned=True))
    cs.append(_case("adam_gscale_half", "adam", lab, n=1027, offset="none", t=11, state="warm", entry="both", clip=1.0, gnorm=5.0, gscale=0.5,
                    aligned=True))
    for bad in ("inf", "nan"):
        cs.append(_case(f"adam_skip_{bad}", "adam", lab, n=1027, offset="none", t=11, state="warm", entry="both", clip=1.0, gnorm=1.0, gscale=1.0,
                        aligned=True, bad=bad))
    return cs


NOAM_WARMUPS = (25, 4000)
ADAM_LR = 1e-3                      # the host entry point's learning rate
NOAM = (1.0, 384.0)                 # base_lr, model_size of the Noam entry point


def adam_entries():
    """(name, lr argument of adam_ref) of the two entry points: a3t_clip_adam, and a3t_clip_adam_noam per warmup."""
    return [("host", ADAM_LR)] + [(f"noam{w}", NOAM + (float(w),)) for w in NOAM_WARMUPS]


def _sumsq_cases():
    cs = []
    for n in (1, 3, 4, 1027):
        for al in (True, False):
            cs.append(_case(f"sumsq_n{n}_{'al' if al else 'off'}", "sumsq", geometry("sumsq", dict(n=n), al)["label"], n=n, aligned=al))
    for n, al in (((1 << 20) + 5, True), ((1 << 20) + 5, False), ((1 << 25) + (1 << 20) + 4, True)):
        cs.append(_case(f"sumsq_n{n}_{'al' if al else 'off'}", "sumsq", geometry("sumsq", dict(n=n), al)["label"], n=n, aligned=al,
                        device_made=n > (1 << 24)))
    return cs


def _dropout_cases():
    cs = []
    for n in DROP_NS:
        lab = geometry("dropout", dict(n=n))["label"]
        for p in DROP_PS:
            for key in DROP_KEYS:
                if n > 1000 and (p, key) not in ((0.1, 0x9e3779b9), (0.5, 0xffffffff), (0.999, 1), (0.0, 0), (1e-6, 0x1234abcd)):
                    continue      # the long one: each p and each key once
                cs.append(_case(f"dropout_n{n}_p{p}_k{key:x}", "dropout", lab, n=n, p=p, key=key, io=("f32", "f32"), scale=1.0))
    lab = geometry("dropout", dict(n=257))["label"]
    cs.append(_case("dropout_f32_bf16", "dropout", lab, n=257, p=0.1, key=0x9e3779b9, io=("f32", "bf16"), scale=1.0))
    cs.append(_case("dropout_bf16_f32", "dropout", lab, n=257, p=0.1, key=0x9e3779b9, io=("bf16", "f32"), scale=1.0))
    cs.append(_case("dropout_scale_half", "dropout", lab, n=257, p=0.5, key=0x1234abcd, io=("f32", "f32"), scale=0.5))
    for M, C in ((1, 1), (5, 63), (129, 65), (300, 256)):
        lab = geometry("dropout_bwd_cast", dict(M=M, C=C))["label"]
        for kind in ("f32", "bf16"):
            for cs_mode in ("none", "zero", "filled"):
                cs.append(_case(f"dropbwd_{M}x{C}_{kind}_{cs_mode}", "dropout_bwd_cast", lab, M=M, C=C, kind=kind, colsum=cs_mode, p=0.1,
                                key=0x9e3779b9 + M, colsum_scale=0.5))
    return cs


def _misc_cases():
    cs = []
    for B, Tm, Tp, D in ((2, 5, 3, 12), (3, 600, 100, 512)):
        n = B * (Tm + Tp) * D
        for seg, spk, p in ((True, True, 0.1), (True, False, 0.0), (False, True, 0.1), (False, False, 0.0), (True, False, 0.1)):
            for op in ("embed_fwd", "embed_bwd"):
                if op == "embed_bwd" and spk and seg:
                    continue      # spk does not enter the backward
                cs.append(_case(f"{op}_{B}x{Tm}x{Tp}x{D}_seg{int(seg)}_spk{int(spk)}_p{p}", op, geometry(op, dict(n=n))["label"], B=B, Tm=Tm,
                                Tp=Tp, D=D, seg=seg, spk=spk, p=p, key=0x1234abcd))
    for N, taps, C in ((1, 1, 1), (80, 5, 256), (256, 5, 80), (33, 3, 31), (384, 1, 384)):
        cs.append(_case(f"cast_conv_t_{N}x{taps}x{C}", "cast_conv_t", geometry("cast_conv_t", dict(N=N, taps=taps, C=C, count=3))["label"], N=N,
                        taps=taps, C=C, count=3))
    # 2^21 + 4 stays below the 8192-block cap (2049 blocks); 2^23 + 4 is the smallest multiple-of-4 class that reaches it
    for n in (4, (1 << 21) + 4, (1 << 23) + 4):
        for op in ("cast_bf16", "split_bf16"):
            cs.append(_case(f"{op}_n{n}", op, geometry(op, dict(n=n))["label"], n=n))
    for B, T, Tm, D in ((1, 1, 1, 1), (3, 9, 5, 12), (2, 700, 640, 384)):
        for kind in ("f32", "bf16"):
            for rev in (False, True):
                cs.append(_case(f"slice_rows_{B}x{T}x{Tm}x{D}_{kind}_{'rev' if rev else 'fwd'}", "slice_rows",
                                geometry("slice_rows", dict(n=B * Tm * D))["label"], B=B, T=T, Tm=Tm, D=D, kind=kind, reverse=rev))
    for n in (1, 257, (1 << 20) + 3):
        for op in ("scale", "scale_dev", "axpy"):
            for inplace in ((False, True) if op != "axpy" else (False,)):
                cs.append(_case(f"{op}_n{n}{'_inplace' if inplace else ''}", op, geometry(op, dict(n=n))["label"], n=n, inplace=inplace))
        for kind in ("f32", "bf16"):
            C = 1 if n == 1 else (257 if n == 257 else 83)
            M = _cdiv(n, C)
            cs.append(_case(f"mask_fill_n{n}_{kind}", "mask_fill", geometry("mask_fill", dict(n=M * C))["label"], M=M, C=C, kind=kind))
        for act in (ACT_NONE, ACT_RELU, ACT_TANH):
            for bias in (True, False):
                for C in ((1,) if n == 1 else (1, 65, 80)):
                    if n > 1000 and (C != 80 or not bias):
                        continue
                    M = _cdiv(n, C)
                    cs.append(_case(f"bias_act_n{n}_C{C}_act{act}_b{int(bias)}", "bias_act", geometry("bias_act", dict(n=M * C))["label"], M=M, C=C,
                                    act=act, bias=bias, scale=0.75))
    for B, T, C in ((1, 1, 1), (3, 5, 65), (2, 1001, 128)):
        cs.append(_case(f"segment_colsum_{B}x{T}x{C}", "segment_colsum", geometry("segment_colsum", dict(B=B, T=T, C=C))["label"], B=B, T=T, C=C))
    for S, d in ((1, 1), (3, 65), (8, 384)):
        cs.append(_case(f"attn_bias_fold_{S}x{d}", "attn_bias_fold", geometry("attn_bias_fold", dict(S=S, d=d))["label"], S=S, d=d))
    for B, Tin, Tout, C in ((3, 300, 200, 7), (3, 300, 310, 80), (4, 5, 9, 3)):
        cs.append(_case(f"splice_spans_{B}x{Tin}x{Tout}x{C}", "splice_spans", geometry("splice_spans", dict(B=B, Tin=Tin, Tout=Tout, C=C))["label"],
                        B=B, Tin=Tin, Tout=Tout, C=C))
    for B, Tm, Tp, P, S, sega in ((3, 300, 7, 6, 2, 1), (3, 5, 300, 4, 1, 1), (2, 9, 4, 0, 2, 1), (2, 9, 4, 3, 0, 0)):
        cs.append(_case(f"collate_paint_{B}x{Tm}x{Tp}_P{P}_S{S}_sega{sega}", "collate_paint",
                        geometry("collate_paint", dict(B=B, Tm=Tm, Tp=Tp))["label"], B=B, Tm=Tm, Tp=Tp, P=P, S=S, sega=sega))
    return cs


CASES = _loss_cases() + _sumsq_cases() + _adam_cases() + _dropout_cases() + _misc_cases()
CASE_BY_ID = {c["id"]: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)

REQUIRED_LABELS = {
    "loss/1row/1lane+ctail", "loss/1row/2lane+ctail", "loss/1row/4lane+ctail", "loss/2rows/2lane+ctail",
    "sumsq/scalar/1trip", "sumsq/vec/1trip", "sumsq/vec+tail/1trip", "sumsq/vec+tail/2trips", "sumsq/scalar/5trips", "sumsq/vec/fold",
    "adam/scalar/1trip", "adam/vec/1trip", "adam/vec+tail/1trip", "adam/scalar/5trips", "adam/vec+tail/2trips",
    "dropout/1trip", "dropout/2trips",
    "dropout_bwd_cast/1x1+ctail", "dropout_bwd_cast/2x2+ctail", "dropout_bwd_cast/4x3",
    "embed_fwd/1trip", "embed_fwd/2trips", "embed_bwd/1trip", "embed_bwd/2trips",
    "cast_conv_t/1tile+nedge+cedge/1tap", "cast_conv_t/tiles+nedge/taps", "cast_conv_t/tiles+cedge/taps", "cast_conv_t/tiles+nedge+cedge/taps",
    "cast_conv_t/tiles/1tap",
    "cast_bf16/1trip", "cast_bf16/cap/2trips", "split_bf16/1trip", "split_bf16/cap/2trips",
    "slice_rows/1trip",
    "scale/1trip", "scale/2trips", "scale_dev/1trip", "scale_dev/2trips", "axpy/1trip", "axpy/2trips",
    "mask_fill/1trip", "mask_fill/2trips", "bias_act/1trip", "bias_act/2trips",
    "segment_colsum/1trip+ctail", "segment_colsum/2trips+ctail", "segment_colsum/251trips",
    "attn_bias_fold/1block", "attn_bias_fold/blocks",
    "splice_spans/1trip/count1/grow", "splice_spans/1trip/count2/shrink", "splice_spans/2trips/count2/grow",
    "collate_paint/2blocks/speech", "collate_paint/2blocks/text", "collate_paint/1block/speech",
}

# entry points of misc.hip in scope -> the ops of the table that call them
ENTRY_POINTS = {
    "a3t_mask_fill": "mask_fill", "a3t_embed_finish_fwd": "embed_fwd", "a3t_embed_finish_bwd": "embed_bwd", "a3t_scale": "scale",
    "a3t_scale_dev": "scale_dev", "a3t_axpy": "axpy", "a3t_attn_bias_fold": "attn_bias_fold", "a3t_cast_bf16": "cast_bf16",
    "a3t_cast_bf16_conv_t": "cast_conv_t", "a3t_split_bf16": "split_bf16", "a3t_slice_rows": "slice_rows", "a3t_mlm_loss": "loss",
    "a3t_sumsq": "sumsq", "a3t_clip_adam": "adam", "a3t_clip_adam_noam": "adam", "a3t_splice_spans": "splice_spans", "a3t_bias_act": "bias_act",
    "a3t_dropout": "dropout", "a3t_dropout_bwd_cast": "dropout_bwd_cast", "a3t_segment_colsum": "segment_colsum",
    "a3t_collate_paint": "collate_paint",
}


def predicted_label(case):
    """The label the geometry gives the case's own sizes (what the table claims is checked against this)."""
    op = case["op"]
    if op in ("adam", "sumsq"):
        return geometry(op, dict(n=case["n"]), case["aligned"])["label"]
    if op in ("embed_fwd", "embed_bwd"):
        return geometry(op, dict(n=case["B"] * (case["Tm"] + case["Tp"]) * case["D"]))["label"]
    if op == "slice_rows":
        return geometry(op, dict(n=case["B"] * case["Tm"] * case["D"]))["label"]
    if op in ("mask_fill", "bias_act"):
        return geometry(op, dict(n=case["M"] * case["C"]))["label"]
    if op == "cast_conv_t":
        return geometry(op, dict(N=case["N"], taps=case["taps"], C=case["C"], count=case["count"]))["label"]
    return geometry(op, case)["label"]


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, 1.00390625, 1.01171875, -1.00390625, 3.3895313892515355e38, -3.4028234663852886e38, np.inf, -np.inf, 1e-40,
                     -1e-45, np.nan, 1.0, 0.333333343267, 65504.0, 1.1754943508222875e-38], dtype=F32)
# (1 + 2^-8 and 1 + 3 * 2^-8 are ties between two bf16 values; 3.3895e38 is the largest finite bf16 and stays, -FLT_MAX rounds to -inf;
#  1e-40 and -1e-45 are fp32 subnormals)


def make_inputs(case):
    """Deterministic host operands of a case (numpy; bf16 operands as torch tensors)."""
    r, op = rng_of(case["id"]), case["op"]
    N = lambda *s: r.standard_normal(s).astype(F32)      # noqa: E731
    if op == "loss":
        M, C = case["M"], case["C"]
        i = dict(before=N(M, C), after=N(M, C) if case["after"] else None, target=N(M, C))
        i["before"][0, 0] = i["target"][0, 0]          # d = 0: the L1 gradient's third branch
        mask = np.ones(M, np.uint8) if case["mask"] == "all" else (np.zeros(M, np.uint8) if case["mask"] == "none" else (r.rand(M) < 0.8).astype(np.uint8))
        if case["mask"] == "most":
            mask[0], mask[-1] = 1, 0
        i["masked"] = mask
        if case.get("nan_unmasked"):
            for k in ("before", "after", "target"):
                i[k][mask == 0] = np.nan
        return i
    if op == "sumsq":
        return dict(g=N(case["n"])) if not case.get("device_made") else {}
    if op == "adam":
        n = case["n"]
        g = N(n)
        g *= F32(case["gnorm"] / max(1e-30, math.sqrt(float((g.astype(np.float64) ** 2).sum()))))
        if case["state"] == "zero":
            p, m, v = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
        else:
            p, m, v = N(n), (0.01 * N(n)).astype(F32), (1e-4 * N(n) ** 2).astype(F32)
        if case.get("bad"):
            g[n // 2] = np.inf if case["bad"] == "inf" else np.nan
        return dict(p=p, g=g, m=m, v=v)
    if op == "dropout":
        x = N(case["n"])
        return dict(x=bf16(x) if case["io"][0] == "bf16" else x)
    if op == "dropout_bwd_cast":
        return dict(g=N(case["M"], case["C"]), colsum0=None if case["colsum"] == "none" else (np.zeros(case["C"], F32) if case["colsum"] == "zero"
                                                                                         else N(case["C"])))
    if op in ("embed_fwd", "embed_bwd"):
        B, Tm, Tp, D = (case[k] for k in ("B", "Tm", "Tp", "D"))
        V, nseg = 11, 7
        e = N(B * Tm, D)
        e[r.rand(B * Tm, D) < 0.1] = 0.0
        text = r.randint(0, V, (B, Tp)).astype(np.int64)
        text[0, 0], text[0, -1], text[-1, 0] = V - 1, 3, 3
        spos, tpos = r.randint(0, nseg, (B, Tm)).astype(np.int64), r.randint(0, nseg, (B, Tp)).astype(np.int64)
        spos[0, 0], tpos[-1, -1] = nseg - 1, nseg - 1
        return dict(e=e, emb=N(V, D), seg=N(nseg, D), text=text, spos=spos, tpos=tpos, spk=N(B, D), dxs=N(B * (Tm + Tp), D), V=V, nseg=nseg,
                    xscale=math.sqrt(D), demb0=N(V, D), dseg0=N(nseg, D))
    if op == "cast_conv_t":
        Nn, taps, C, cnt = case["N"], case["taps"], case["C"], case["count"]
        sz = Nn * taps * C
        gap = 4 - sz % 4                                                              # every source offset is 1 modulo 4 floats:
        src_off = np.array([1 + k * (sz + gap) for k in range(cnt)], np.int64)        # none is 16-byte aligned
        dst_off = np.array([5 + k * (sz + 7) for k in range(cnt)], np.int64)
        return dict(src=N(1 + cnt * (sz + gap)), src_off=src_off, dst_off=dst_off, dst_len=5 + cnt * (sz + 7))
    if op in ("cast_bf16", "split_bf16"):
        x = N(case["n"])
        x[:4] = SPECIALS[[0, 1, 2, 5]]
        if case["n"] > 16:
            x[-16:] = SPECIALS
            x[16:32] = SPECIALS[::-1]
        return dict(x=x)
    if op == "slice_rows":
        B, T, Tm, D = (case[k] for k in ("B", "T", "Tm", "D"))
        y = N(B * Tm, D)
        return dict(x=N(B * T, D), y=bf16(y) if case["kind"] == "bf16" else y)
    if op in ("scale", "scale_dev", "axpy"):
        return dict(x=N(case["n"]), y=N(case["n"]), s=0.37)
    if op == "mask_fill":
        M, C = case["M"], case["C"]
        m = (r.rand(M) < 0.5).astype(np.uint8)
        m[0], m[-1] = 1, (0 if M > 1 else 1)
        return dict(x=N(M, C), mf=N(C), masked=m)
    if op == "bias_act":
        return dict(x=(2 * N(case["M"], case["C"])).astype(F32), bias=N(case["C"]) if case["bias"] else None)
    if op == "segment_colsum":
        return dict(x=N(case["B"] * case["T"], case["C"]), out0=N(case["B"], case["C"]))
    if op == "attn_bias_fold":
        S, d = case["S"], case["d"]
        return dict(slots=N(S, 4 * d), gu0=N(d), gv0=N(d), gb0=N(3 * d))
    if op == "splice_spans":
        B, Tin, Tout, C = (case[k] for k in ("B", "Tin", "Tout", "C"))
        mask = np.zeros((B, Tin), np.uint8)
        lens = [Tin, max(1, Tin // 2), 0] + [max(1, Tin - 1)] * (B - 3)
        for b in range(B):
            mask[b, :lens[b]] = 1
        spans = np.array([[2, 2], [Tin // 4, Tin + 50], [0, 3]] + [[1, 3]] * (B - 3), np.int32)      # empty; past the length; all-zero row
        return dict(after=N(B, Tin, C), speech=N(B, Tin, C), mask=mask, spans=spans)
    if op == "collate_paint":
        B, Tm, Tp, P, S = (case[k] for k in ("B", "Tm", "Tp", "P", "S"))
        fs = np.sort(r.randint(0, Tm, (B, max(P, 1))), axis=1).astype(np.int32)[:, :P]
        fe = (fs + r.randint(1, max(2, Tm // 2), (B, P))).astype(np.int32)            # long phones: they overlap, the later one wins
        alen = np.array([P + 2, max(0, P - 1)] + [P] * (B - 2), np.int32)[:B]        # alen > P, alen < P
        flen = np.array([Tm, max(1, Tm - 2)] + [Tm // 2] * (B - 2), np.int32)[:B]
        tlen = np.array([Tp, max(0, Tp - 1)] + [Tp // 2] * (B - 2), np.int32)[:B]
        ms = np.sort(r.randint(0, Tm + 1, (B, max(S, 1), 2)), axis=2).astype(np.int32)[:, :S]
        nms = np.array([S, max(0, S - 1)] + [S] * (B - 2), np.int32)[:B]
        return dict(fs=fs.reshape(B, P), fe=fe.reshape(B, P), alen=alen, sel=(r.rand(B, P) < 0.5).astype(np.uint8), mspan=ms.reshape(B, S, 2),
                    nms=nms, flen=flen, tlen=tlen)
    raise KeyError(op)
