"""A descriptor interpreter for a3t_gemm and an integer case generator (CPU only).

reference() restates the contract of include/a3t_hip.h by explicit index gathers in float64: every operand element is fetched
through the strides of the descriptor, so a test that compares a kernel against it checks indexing, masking and the epilogue
rather than a reshaped torch call.  The generator fills operands with small integers (and alpha with a power of two) such that
every product, partial sum and column sum is an exactly representable integer multiple of a power of two below 2^24: in fp32 and
in bf16-in / fp32-accumulate, under any accumulation order, the kernel's result must then EQUAL the reference.
"""
import collections
import random

import torch

from a3t_amd._lib import (ACC_ADD, ACC_ATOMIC, ACC_SOLE, ACC_STORE, ACT_NONE, ACT_RELU, ACT_SWISH, ACT_TANH, BF16, F32)

EXACT = float(1 << 24)
POS = ("M", "N", "K", "a_rs", "a_cs", "b_rs", "b_cs", "c_rs")
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
BB, BF = ("bf16", "bf16", "bf16"), ("bf16", "bf16", "f32")      # storage of A, B, C

Ref = collections.namedtuple("Ref", "C colsum colsum2 mag")


def _base(t):
    """(flat view of the whole storage under t, element offset of t[0] in it)"""
    n = t.untyped_storage().nbytes() // t.element_size()
    return t.as_strided((n,), (1,), 0), t.storage_offset()


def _gather(t, idx, ok=None, signmask=False):
    """float64 values t[idx] (idx relative to t's first element, may be negative) where ok, 0 elsewhere"""
    flat, off = _base(t)
    idx = idx + off
    if ok is None:
        ok = torch.ones(idx.shape, dtype=torch.bool)
    ok = ok.expand(idx.shape)
    sel = idx[ok]
    if sel.numel():
        assert int(sel.min()) >= 0 and int(sel.max()) < flat.numel(), "the descriptor reads outside its operand"
    vals = flat[sel]
    if signmask:       # elements with the sign bit set (-0 included) are read as zero
        vals = torch.where(torch.signbit(vals), torch.zeros_like(vals), vals)
    out = torch.zeros(idx.shape, dtype=torch.float64)
    out[ok] = vals.to(torch.float64)
    return out


def _act(v, act):
    if act == ACT_RELU:
        return v.clamp(min=0)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SWISH:
        return v * torch.sigmoid(v)
    assert act == ACT_NONE
    return v


def reference(kw, A, B, C_old, bias=None, R=None, S=None, keep=None, A2=None, B2=None):
    """What a3t_gemm leaves behind for the descriptor `kw` (the arguments of ops._gemm_desc by name, tensors apart; `second` as a
    dict b2_cs / b2_bs / a2_rs).  A, B, C_old, R, S, keep, A2, B2: CPU tensors whose element 0 is the descriptor's pointer (tail
    views of larger buffers are fine: negative strides reach in front of them).  keep: the dropout keep mask (> 0: kept) by
    linear index in C.  Returns Ref(C: float64 image of C_old's extent afterwards, colsum / colsum2: the increments a zeroed
    accumulator receives, slots folded, or None; mag: |alpha| (sum |a||b| + |bias|) + |R| + |C_old| per element of C)."""
    g = kw.get
    M, N, K = kw["M"], kw["N"], kw["K"]
    a_rs, a_cs, b_rs, b_cs, c_rs = (kw[k] for k in POS[3:])
    b_ts = g("b_ts", 0)
    taps, pad, dil, Tseq, kshift = max(1, g("taps", 1)), g("pad", 0), max(1, g("dil", 1)), g("Tseq", 0), g("kshift", 0)
    batch, bi = max(1, g("batch", 1)), max(1, g("batch_inner", 1))
    a_bs, b_bs, c_bs = g("a_bs", (0, 0)), g("b_bs", (0, 0)), g("c_bs", (0, 0))
    alpha, act, acc, splitk = g("alpha", 1.0), g("act", ACT_NONE), g("acc", ACC_STORE), max(1, g("splitk", 1))
    drop, second = g("drop"), g("second")
    if (a_cs != 1 and a_rs != 1) or (b_cs != 1 and b_rs != 1):
        raise ValueError("one of a_rs / a_cs and of b_rs / b_cs must be 1")
    if splitk > 1 and (acc not in (ACC_ATOMIC, ACC_SOLE) or act != ACT_NONE):
        raise ValueError("split K needs an atomic accumulate and a linear epilogue")
    if taps > 1 and Tseq <= 0:
        raise ValueError("taps need Tseq")
    m, k, n = torch.arange(M)[:, None], torch.arange(K)[None, :], torch.arange(N)[:, None]
    inside = lambda t: (t >= 0) & (t < Tseq)
    a_ok = b_ok = None
    if taps > 1 and a_cs == 1:          # implicit im2col: k = (tap, c), zero padding per utterance
        if K % taps:
            raise ValueError("K % taps")
        Kc = K // taps
        tap, c = k // Kc, k % Kc
        off = (tap - pad) * dil
        a_idx, a_ok = (m + off) * a_rs + c, inside(m % Tseq + off)
        b_idx = n * b_rs + tap * b_ts + c * b_cs
    elif taps > 1:                      # fused conv weight gradient: output columns n = (tap, c), tokens k shifted per tap
        if N % taps:
            raise ValueError("N % taps")
        Cn = N // taps
        off = (n // Cn - pad) * dil
        a_idx = m * a_rs + k * a_cs
        b_idx, b_ok = (n % Cn) * b_rs + (k + off) * b_cs, inside(k % Tseq + off)
    else:
        a_idx = m * a_rs + k * a_cs
        if Tseq > 0:                    # token-reduction GEMM with one token shift
            b_idx, b_ok = n * b_rs + (k + kshift) * b_cs, inside(k % Tseq + kshift)
        else:
            b_idx = n * b_rs + k * b_cs
    c_idx = m * c_rs + torch.arange(N)[None, :]
    c_flat = C_old.reshape(-1)
    out = c_flat.to(torch.float64).clone()
    mag = torch.zeros_like(out)
    cs = cs2 = None
    if g("colsum_len"):
        cs = torch.zeros(g("colsum_len"), dtype=torch.float64)
        cs2 = torch.zeros_like(cs) if second else None
    bias64 = bias.to(torch.float64)[None, :N] if bias is not None else None
    for z in range(batch):
        z0, z1 = divmod(z, bi)
        Az = _gather(A, a_idx + z0 * a_bs[0] + z1 * a_bs[1], a_ok, bool(g("a_signmask")))
        Bz = _gather(B, b_idx + z0 * b_bs[0] + z1 * b_bs[1], b_ok)
        first = Az @ Bz.t()
        absum = Az.abs() @ Bz.abs().t()
        v = first
        if second:
            a2_idx = m * (second.get("a2_rs") or a_rs) + k * a_cs + z0 * a_bs[0] + z1 * a_bs[1]
            b2_idx = k.t() * second["b2_cs"] + torch.arange(N)[None, :] + z0 * second["b2_bs"][0] + z1 * second["b2_bs"][1]
            A2z, B2z = _gather(A2, a2_idx), _gather(B2, b2_idx)
            v = first + A2z @ B2z
            absum = absum + A2z.abs() @ B2z.abs()
        if bias64 is not None:
            v = v + bias64
            absum = absum + bias64.abs()
        v = _act(v, act)
        idx = c_idx + z0 * c_bs[0] + z1 * c_bs[1]
        if S is not None:
            v = torch.where(_gather(S, idx) > 0, v, torch.zeros_like(v))
        if drop is not None and drop[0] > 0:
            v = torch.where(_gather(keep, idx) > 0, v / (1.0 - drop[0]), torch.zeros_like(v))
        v = v * alpha
        absum = absum * abs(alpha)
        if R is not None:
            r = _gather(R, idx)
            v, absum = v + r, absum + r.abs()
        if cs is not None:
            o = z1 * g("colsum_bs1", 0)
            if second:
                f = (alpha * first).sum(0) * g("colsum_scale", 1.0)
                cs[o:o + N] += f
                cs2[o:o + N] += v.sum(0) * g("colsum_scale", 1.0) - f
            else:
                cs[o:o + N] += v.sum(0) * g("colsum_scale", 1.0)
        assert int(idx.min()) >= 0 and int(idx.max()) < out.numel(), "the descriptor writes outside C"
        old = out[idx]
        new = v if acc == ACC_STORE else old + v
        if C_old.dtype == torch.bfloat16:       # the sum is formed in fp32 and rounded once
            new = new.to(torch.float32).to(torch.bfloat16).to(torch.float64)
        out[idx] = new
        mag[idx] = absum + old.abs()
    return Ref(out.view(C_old.shape), cs, cs2, mag.view(C_old.shape))


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case:
    """One descriptor with its operands.  kw: the descriptor by name (no tensors); bufs: name -> (flat CPU buffer, offset of the
    descriptor's pointer in it) for A, B, C, bias, R, S, A2, B2, colsum, colsum2."""

    def __init__(self, name, kw, bufs):
        self.name, self.kw, self.bufs = name, kw, bufs

    def place(self, dev="cpu"):
        """(name -> tensor whose element 0 is the descriptor's pointer, name -> the whole buffer), copied to dev"""
        base = {k: (b.clone() if dev == "cpu" else b.to(dev)) for k, (b, _) in self.bufs.items()}
        return {k: base[k][off:] for k, (_, off) in self.bufs.items()}, base

    def call(self, fn, t):
        """fn = ops.gemm or ops.gemm_plan on the placed tensors t"""
        k = {x: v for x, v in self.kw.items() if x not in POS and x != "colsum_len"}
        sec = k.pop("second", None)
        if sec:
            k["second"] = (t["A2"], t["B2"], sec["b2_cs"], sec["b2_bs"], t.get("colsum2")) + ((sec["a2_rs"],) if sec.get("a2_rs") else ())
        for nm in ("bias", "R", "S", "colsum"):
            if nm in t:
                k[nm] = t[nm]
        return fn(t["A"], t["B"], t["C"], *(self.kw[x] for x in POS), **k)

    def reference(self, t, keep=None):
        return reference(self.kw, t["A"], t["B"], t["C"], bias=t.get("bias"), R=t.get("R"), S=t.get("S"), keep=keep,
                         A2=t.get("A2"), B2=t.get("B2"))

    def __repr__(self):
        return f"{self.name} {self.kw}"


def _span(*dims):
    """elements spanned by an index set: 1 + sum (count - 1) * stride"""
    return 1 + sum((c - 1) * s for c, s in dims)


def _bs(kind, span, outer, inner, gap=0):
    """(bs0, bs1) of a two-level batch: 'dense' z1 fastest, 'swap' z0 fastest (head-major), 'shared' none, or a given pair"""
    if isinstance(kind, tuple):
        return kind
    if kind == "shared":
        return (0, 0)
    step = span + gap
    return (inner * step + gap, step) if kind == "dense" else (step, outer * step + gap)


def build(name, seed, M, N, K, layout="NT", compute=F32, dt=("f32", "f32", "f32"), a_ld=None, b_ld=None, c_ld=None, offs=(0, 0, 0),
          batch=1, batch_inner=1, a_bs="dense", b_bs="dense", c_bs="dense", bs_gap=0, taps=1, pad=0, dil=1, Tseq=0, kshift=0,
          bias=False, R=False, S=None, alpha=1.0, act=ACT_NONE, acc=ACC_STORE, splitk=1, colsum=False, colsum_scale=1.0,
          colsum_slots=1, drop=None, signmask=False, second=False, a2_rs=None, a_view=False, values="int", tail=8):
    """A Case.  layout NT: A [m][k] x B [n][k]; NN: A [m][k] x B [k][n] (with taps: the conv data gradient, taps read back to
    front through b_ts < 0); TN: A [k][m] x B [k][n] (with taps: the fused conv weight gradient, N = taps * channels).  a_ld /
    b_ld / c_ld: the leading strides (default: dense; a_ld < K: overlapping rows).  offs: element offsets of the A, B, C pointers
    in their buffers.  values 'int': the exact-integer fill, narrowed until every accumulated quantity is below 2^24; 'gauss':
    standard normal operands."""
    gen = torch.Generator().manual_seed(seed)
    conv = taps > 1 and layout != "TN"
    wgrad = taps > 1 and layout == "TN"
    Kc = K // taps if conv else K
    Cn = N // taps if wgrad else N
    kw = dict(M=M, N=N, K=K, compute=compute)
    bufs = {}
    # strides and spans of one batch element
    if layout in ("NT", "NN"):
        a_rs, a_cs = (a_ld if a_ld is not None else Kc), 1
        a_span = _span((M, a_rs), (Kc, 1))
    else:
        a_rs, a_cs = 1, (a_ld if a_ld is not None else M)
        a_span = _span((K, a_cs), (M, 1))
    b_off = offs[1]
    b_ts = 0
    if layout == "NT":
        b_rs, b_cs = (b_ld if b_ld is not None else K), 1
        b_span = _span((N, b_rs), (K, 1))
        b_ts = Kc if conv else 0
    elif conv:                                  # B = W[co][tap][ci] read as W^T with the taps reversed
        b_rs, b_cs, b_ts = 1, taps * N, -N
        b_span = _span((Kc, b_cs), (taps, N), (N, 1))
        b_off += (taps - 1) * N
    else:
        b_rs, b_cs = 1, (b_ld if b_ld is not None else (Cn if Cn > 1 or layout == "NN" else 2))     # ([k][m] x [n][k] does not exist)
        b_span = _span((K, b_cs), (Cn, 1))
    c_rs = c_ld if c_ld is not None else N
    c_span = M * c_rs
    kw.update(a_rs=a_rs, a_cs=a_cs, b_rs=b_rs, b_cs=b_cs, c_rs=c_rs)
    outer = (batch + batch_inner - 1) // batch_inner
    if batch > 1:
        kw.update(batch=batch, batch_inner=batch_inner, a_bs=_bs(a_bs, a_span, outer, batch_inner, bs_gap),
                  b_bs=_bs(b_bs, b_span, outer, batch_inner, bs_gap), c_bs=_bs(c_bs, c_span, outer, batch_inner, bs_gap))
    zmax = lambda bs: (outer - 1) * bs[0] + (batch_inner - 1) * bs[1] if batch > 1 else 0
    if b_ts:
        kw["b_ts"] = b_ts
    if taps > 1:
        kw.update(taps=taps, pad=pad, dil=dil, Tseq=Tseq)
    elif Tseq > 0:
        kw.update(Tseq=Tseq, kshift=kshift)
    if alpha != 1.0:
        kw["alpha"] = alpha
    if act != ACT_NONE:
        kw["act"] = act
    if acc != ACC_STORE:
        kw["acc"] = acc
    if splitk > 1:
        kw["splitk"] = splitk
    if drop is not None:
        kw["drop"] = drop
    if signmask:
        kw["a_signmask"] = True
    if a_view:
        kw["a_view"] = True
    # magnitudes: narrow the operand range until C, the split-K partials (bounded by C's bound) and the column sums over all rows
    # of a slot stay exact
    amax, bmax = 3, 3
    rows = M * (outer if batch > 1 else 1)
    while values == "int":
        v = abs(alpha) * ((2 if second else 1) * K * amax * bmax + (8 if bias else 0)) * (2 if drop else 1) + (8 if R else 0)
        unit = min(1.0, abs(alpha))
        worst = (v + 8) / unit
        if colsum:
            worst = max(worst, abs(colsum_scale) * rows * v / (unit * min(1.0, abs(colsum_scale))))
        if worst < EXACT:
            break
        if amax > 1:
            amax -= 1
        elif bmax > 1:
            bmax -= 1
        else:
            raise RuntimeError(f"{name}: no integer range keeps the sums below 2^24")

    def fill(n, hi, dtype):
        if values == "int":
            return torch.randint(-hi, hi + 1, (n,), generator=gen).to(dtype)
        return torch.randn(n, generator=gen).to(dtype)

    a_dt, b_dt, c_dt = (TDT[x] for x in dt)
    A = fill(offs[0] + zmax(kw.get("a_bs", (0, 0))) + a_span + tail, amax, a_dt)
    if signmask:
        A = torch.where(torch.rand(A.shape, generator=gen) < 0.1, torch.full_like(A, -0.0), A)
    bufs["A"] = (A, offs[0])
    bufs["B"] = (fill(b_off + zmax(kw.get("b_bs", (0, 0))) + b_span + tail, bmax, b_dt), b_off)
    c_len = offs[2] + zmax(kw.get("c_bs", (0, 0))) + c_span + tail
    bufs["C"] = (fill(c_len, 8, c_dt), offs[2])
    if bias:
        bufs["bias"] = (fill(N, 8, torch.float32), 0)
    if R:
        bufs["R"] = (fill(c_len, 8, torch.float32), offs[2])
    if S:
        bufs["S"] = ((torch.randint(-1, 3, (c_len,), generator=gen) if values == "int" else torch.randn(c_len, generator=gen)).to(TDT[S]), offs[2])
    if second:
        b2_span = K * N
        sec = dict(b2_cs=N, b2_bs=_bs("dense", b2_span, outer, batch_inner) if batch > 1 else (0, 0))
        if a2_rs:
            sec["a2_rs"] = a2_rs
        kw["second"] = sec
        a2_span = _span((M, a2_rs or a_rs), (K, 1))
        bufs["A2"] = (fill(zmax(kw.get("a_bs", (0, 0))) + a2_span + tail, amax, a_dt), 0)
        bufs["B2"] = (fill(zmax(sec["b2_bs"]) + b2_span + tail, bmax, b_dt), 0)
    if colsum:
        bs1 = (N + 3) // 4 * 4 + 4 if batch_inner > 1 else 0
        ss = (batch_inner - 1) * bs1 + N
        kw.update(colsum_len=ss, colsum_bs1=bs1, colsum_scale=colsum_scale)
        if colsum_slots > 1:
            ss = (ss + 3) // 4 * 4
            kw.update(colsum_slots=colsum_slots, colsum_ss=ss)
        bufs["colsum"] = (torch.zeros(ss * colsum_slots), 0)
        if second:
            bufs["colsum2"] = (torch.zeros(ss * colsum_slots), 0)
    return Case(name, kw, bufs)


def folded(case, colsum):
    """the slot copies of a column-sum accumulator summed (float64)"""
    n = case.kw["colsum_len"]
    slots = case.kw.get("colsum_slots", 1)
    ss = case.kw.get("colsum_ss", n)
    return colsum.to(torch.float64).cpu().view(slots, ss)[:, :n].sum(0)


# ---- the fixed fp32 table (issue: the smallest shapes at which the 128 x 128 x 16 tiling can go wrong) -----------------------
F32_M = (1, 37, 127, 128, 129, 200)
F32_K = (1, 3, 15, 16, 17, 24, 33, 130)
POW2 = (1.0, 0.5, -2.0, 0.25)


def f32_shape_cases(layout):
    """every K x every M, N walking the same list two steps ahead and then one behind: each (M, K) and each (N, K) occurs"""
    out = []
    for ki, K in enumerate(F32_K):
        for mi, M in enumerate(F32_M):
            for N in (F32_M[(mi + 2 + ki) % 6], F32_M[(mi + 5 + ki) % 6]):
                out.append(build(f"{layout} {M}x{N}x{K}", 1000 * ki + 10 * mi + N, M, N, K, layout))
    return out


def f32_stride_cases():
    c = []
    for i, ly in enumerate(("NT", "NN", "TN")):
        # leading strides larger than the dense ones, vector (multiples of 4, 16-byte pointers) and scalar
        c.append(build(f"{ly} wide rows vec", 10 + i, 129, 37, 24, ly, a_ld=132 if ly == "TN" else 28, b_ld=40, c_ld=44, offs=(4, 8, 4)))
        c.append(build(f"{ly} wide rows scalar", 20 + i, 129, 37, 17, ly, a_ld=131 if ly == "TN" else 19, b_ld=39, c_ld=41, offs=(1, 3, 5)))
        c.append(build(f"{ly} batch 6/3", 30 + i, 37, 129, 16, ly, batch=6, batch_inner=3, a_bs="swap", b_bs="dense", c_bs="swap", bs_gap=4))
        c.append(build(f"{ly} batch 6/3 scalar", 40 + i, 37, 40, 15, ly, batch=6, batch_inner=3, a_bs="dense", b_bs="swap", c_bs="dense", bs_gap=3))
    # overlapping rows: the STFT framing (frame m starts hop samples behind frame m - 1)
    c.append(build("overlap hop 3", 50, 200, 37, 16, "NT", a_ld=3))
    c.append(build("overlap hop 4", 51, 200, 37, 16, "NT", a_ld=4))
    c.append(build("overlap hop 4 batched", 52, 129, 130, 16, "NT", a_ld=4, batch=3, b_bs="shared"))
    # one B for all heads of a batch element: b_bs = (0, dk)
    c.append(build("shared B (0, dk)", 53, 37, 16, 33, "NN", b_ld=48, batch=6, batch_inner=3, b_bs=(0, 16)))
    # C is a column slice of a wider tensor
    c.append(build("C slice", 54, 129, 37, 24, "NT", c_ld=64, offs=(0, 0, 16)))
    c.append(build("C slice odd", 55, 130, 127, 33, "NN", c_ld=150, offs=(0, 0, 7)))
    return c


def f32_conv_cases():
    c, s = [], 100
    for taps in (3, 5):
        for dil in (1, 2, 4):
            for Tseq in (1, 3, 7, 50):
                for pad in (0, (taps - 1) // 2, taps - 1):
                    s += 1
                    Cin, N = (4, 37) if s % 2 else (3, 129)       # vector and scalar loaders
                    c.append(build(f"conv k{taps} d{dil} T{Tseq} p{pad}", s, 3 * Tseq, N, taps * Cin, "NT", taps=taps, pad=pad,
                                   dil=dil, Tseq=Tseq))
                    if pad == (taps - 1) // 2:      # the data gradient: Cout = 8 -> Cin = 4 (vector) and 7 -> 5 (scalar)
                        Ci, Co = (4, 8) if s % 2 else (5, 7)
                        c.append(build(f"conv_bwd_data k{taps} d{dil} T{Tseq}", s + 500, 3 * Tseq, Ci, taps * Co, "NN",
                                       taps=taps, pad=taps - 1 - pad, dil=dil, Tseq=Tseq))
    return c


def f32_acc_cases():
    c, s = [], 2000
    for Tseq in (7, 50):
        for kshift in (-2, 0, 3, Tseq, -Tseq):
            s += 1
            c.append(build(f"kshift {kshift} T{Tseq}", s, 37, 129 if s % 2 else 40, 3 * Tseq, "TN", Tseq=Tseq, kshift=kshift, acc=ACC_ATOMIC,
                           splitk=2 if Tseq == 50 else 1, alpha=POW2[s % 4]))
    for ly in ("NT", "NN", "TN"):
        for acc in (ACC_ADD, ACC_ATOMIC, ACC_SOLE):
            for splitk in ((1,) if acc == ACC_ADD else (1, 2, 5)):
                s += 1
                # 130 -> 9 K-tiles: 5 splits of 2 tiles leave the last one a single tile; 97 -> 7 tiles: 5 splits of 2, the last EMPTY
                K = (130, 97, 96)[s % 3] if splitk == 5 else (33, 130)[s % 2]
                c.append(build(f"{ly} acc {acc} splitk {splitk} K{K}", s, 129, 37, K, ly, acc=acc, splitk=splitk, alpha=POW2[s % 4],
                               bias=s % 2 == 0, R=s % 3 == 0, S=(None, "f32", "bf16")[s % 3]))
    c.append(build("empty last split", s + 1, 37, 37, 97, "NT", acc=ACC_ATOMIC, splitk=5))
    return c


def f32_epilogue_cases():
    c, s = [], 3000
    for ly in ("NT", "NN", "TN"):
        for S in ("f32", "bf16"):
            s += 1
            c.append(build(f"{ly} bias relu S {S} alpha R", s, 129, 130, 24, ly, bias=True, act=ACT_RELU, S=S, alpha=POW2[1 + s % 3], R=True))
            c.append(build(f"{ly} epilogue scalar {S}", s + 50, 37, 127, 17, ly, bias=True, act=ACT_RELU, S=S, alpha=-2.0, R=True,
                           c_ld=129, offs=(0, 0, 1)))
        for acc in (ACC_STORE, ACC_ADD):
            s += 1
            c.append(build(f"{ly} bf16 C acc {acc}", s + 100, 129, 37, 33 if acc else 130, ly, dt=("f32", "f32", "bf16"), acc=acc, bias=True,
                           alpha=0.5 if acc else 1.0))
    c.append(build("conv epilogue", s + 200, 21, 37, 12, "NT", taps=3, pad=1, dil=2, Tseq=7, bias=True, act=ACT_RELU, S="bf16", alpha=0.5, R=True))
    c.append(build("dropout", s + 201, 129, 40, 24, "NT", drop=(0.5, 4321), bias=True, alpha=0.5))
    return c


def f32_fixed_cases():
    return (f32_shape_cases("NT") + f32_shape_cases("NN") + f32_shape_cases("TN") + f32_stride_cases() + f32_conv_cases() +
            f32_acc_cases() + f32_epilogue_cases())


# ---- seeded random descriptors -----------------------------------------------------------------------------------------------
def draw(rng, compute, i=0):
    """One random descriptor over the whole space the compute mode accepts: layouts, strides, batches, conv forms, token shifts,
    accumulate modes with split K, epilogues.  bf16 draws keep the 8-element granules of the bf16 kernels."""
    f32 = compute == F32
    if not f32 and rng.random() < 0.35:
        return _route_draw(rng, i)
    q = rng.choice((1, 4)) if f32 else 8       # (fp32: half of the draws keep the 16-byte granules of the vector loaders)
    dim = lambda lo, hi: q * rng.randrange(max(1, lo // q), hi // q + 1)
    seed = rng.randrange(1 << 30)
    ly = rng.choice(("NT", "NN", "TN"))
    fam = rng.choice(("plain", "plain", "strided", "batched", "conv", "kshift", "overlap"))
    M, N, K = dim(1, 300), dim(1, 300), dim(1, 200)
    k = dict(layout=ly, compute=compute)
    if f32:
        k["dt"] = ("f32", "f32", rng.choice(("f32", "f32", "bf16")))
    else:
        k["dt"] = rng.choice((("bf16", "bf16", "bf16"), ("bf16", "bf16", "f32"), ("bf16", "bf16", "bf16"), ("bf16", "bf16", "f32"),
                              ("f32", "bf16", "f32"), ("bf16", "f32", "bf16"), ("f32", "f32", "f32")))
        if rng.random() < 0.4:      # whole K-tiles of the persistent kernels
            K = 64 * rng.randrange(1, 5)
    rup = lambda v, to: (v + to - 1) // to * to
    if fam == "strided":
        g = q
        lead = {"NT": (K, K), "NN": (K, N), "TN": (M, N)}[ly]
        k.update(a_ld=rup(lead[0] + rng.randrange(1, 9), g), b_ld=rup(lead[1] + rng.randrange(1, 9), g), c_ld=rup(N + rng.randrange(1, 9), 4 if not f32 else g),
                 offs=tuple(g * rng.randrange(0, 3) for _ in range(3)))
    elif fam == "batched":
        M, N = min(M, 136), min(N, 136)
        inner = rng.choice((1, 2, 3))
        k.update(batch=inner * rng.choice((1, 2, 3)), batch_inner=inner, a_bs=rng.choice(("dense", "swap")), b_bs=rng.choice(("dense", "swap", "shared")),
                 c_bs=rng.choice(("dense", "swap")), bs_gap=q * rng.randrange(0, 3))
    elif fam == "conv":
        taps, Tseq = rng.choice((3, 5)), rng.choice((1, 3, 7, 50, 64))
        Bn = rng.randrange(1, 5)
        ly = rng.choice(("NT", "NN"))
        ch = dim(1, 40)
        M, K = Bn * Tseq, taps * ch
        if not f32 and ly == "NN":
            N = rup(N, 8)
        k.update(layout=ly, taps=taps, dil=rng.choice((1, 2, 4)), Tseq=Tseq, pad=rng.choice((0, (taps - 1) // 2, taps - 1)))
        if not f32:         # the bf16 kernels want whole 8-row granules
            M = Bn * Tseq if (Bn * Tseq) % 8 == 0 else 8 * Tseq
    elif fam == "kshift":
        Tseq = rng.choice((3, 7, 50, 64))
        ly, K = "TN", Tseq * rng.randrange(1, 5) * (1 if f32 else 8)
        k.update(layout=ly, Tseq=Tseq, kshift=rng.choice((-2, -1, 0, 1, 3, Tseq, -Tseq)))
    elif fam == "overlap":
        ly, K = "NT", dim(8, 64)
        k.update(layout=ly, a_ld=rng.choice(((1, 3, 5), (4, 8), (8, 16))[(q > 1) + (q > 4)]))
    # epilogue and accumulate mode
    c_bf16 = k["dt"][2] == "bf16"
    acc = rng.choice((ACC_STORE, ACC_STORE, ACC_ADD) if c_bf16 else (ACC_STORE, ACC_STORE, ACC_ADD, ACC_ATOMIC, ACC_SOLE))
    if fam == "kshift" and not c_bf16:
        acc = rng.choice((ACC_ATOMIC, ACC_SOLE))
    splitk = rng.choice((1, 2, 3, 5)) if acc in (ACC_ATOMIC, ACC_SOLE) else 1
    k.update(acc=acc, splitk=splitk, alpha=rng.choice(POW2), bias=rng.random() < 0.4, R=rng.random() < 0.3,
             S=rng.choice((None, None, "f32", "bf16")), act=ACT_RELU if splitk == 1 and rng.random() < 0.4 else ACT_NONE)
    if rng.random() < 0.15:
        k["drop"] = (0.5, rng.randrange(1, 1 << 20))
    if not f32 and k["dt"][:2] == ("bf16", "bf16") and acc != ACC_ATOMIC and rng.random() < 0.3 and N % 4 == 0:
        k.update(colsum=True, colsum_scale=rng.choice(POW2), colsum_slots=rng.choice((1, 1, 4)))
        if fam == "strided":
            k["c_ld"] = rup(k["c_ld"], 4)
            k["offs"] = tuple(rup(o, 8) for o in k["offs"])
    return build(f"draw{i} {fam} {k['layout']} {M}x{N}x{K}", seed, M, N, K, **k)


def _route_draw(rng, i):
    """a bf16 descriptor inside the contracts of the persistent, panel, token-reduction and streaming kernels: which one runs it
    is up to the mode setters"""
    seed = rng.randrange(1 << 30)
    kind = rng.choice(("nt", "nt", "conv", "tn", "tt"))
    if kind in ("nt", "conv"):
        M, N, K = 8 * rng.randrange(17, 66), rng.choice((72, 136, 264, 384)), 128 * rng.randrange(1, 3)
        k = dict(dt=rng.choice((BB, BF)), bias=rng.random() < 0.5, act=rng.choice((ACT_NONE, ACT_RELU)), R=rng.random() < 0.3, alpha=rng.choice(POW2),
                 S=rng.choice((None, None, "bf16")), colsum=rng.random() < 0.3)
        if rng.random() < 0.2:
            k["drop"] = (0.5, rng.randrange(1, 1 << 20))
        if kind == "conv":
            taps, Tseq = rng.choice((3, 5)), rng.choice((7, 56))
            M, K = Tseq * rng.randrange(2, 5), taps * rng.choice((64, 128))
            k.update(taps=taps, pad=rng.randrange(taps), dil=rng.choice((1, 2)), Tseq=Tseq)
        return build(f"draw{i} route {kind} {M}x{N}x{K}", seed, M, N, K, "NT", compute=BF16, **k)
    if kind == "tn":
        M, N, K = 8 * rng.randrange(1, 40), 8 * rng.randrange(1, 50), 8 * rng.randrange(1, 60)
        return build(f"draw{i} route tn {M}x{N}x{K}", seed, M, N, K, "TN", compute=BF16, dt=BF, acc=rng.choice((ACC_STORE, ACC_ADD, ACC_ATOMIC, ACC_SOLE)),
                     alpha=rng.choice(POW2))
    ly = rng.choice(("NN", "TN"))
    M, N, K = 8 * rng.randrange(1, 80), 8 * rng.randrange(1, 25), 8 * rng.randrange(1, 30)
    batch = rng.choice((1, 2, 4))
    return build(f"draw{i} route tt {ly} {M}x{N}x{K}", seed, M, N, K, ly, compute=BF16, dt=BB, acc=rng.choice((ACC_STORE, ACC_ADD)), alpha=rng.choice(POW2),
                 batch=batch, batch_inner=min(batch, rng.choice((1, 2))), colsum=rng.random() < 0.4, signmask=ly == "TN" and rng.random() < 0.3)


def draws(seed, n, compute):
    rng = random.Random(seed)
    return [draw(rng, compute, i) for i in range(n)]


# ---- the bf16 routes: smallest shapes each route's plan accepts when its mode setter forces it --------------------------------
# (a3t_gemm_8p_mode, _pn_mode, _tt_mode, _tn3_mode): 0 never, 1 whenever legal, 2 the cost model
MODES = {"off": (0, 0, 0, 0), "8p": (1, 0, 0, 0), "tn3": (1, 0, 0, 1), "pn": (0, 1, 0, 0), "tt": (0, 0, 1, 0), "default": (2, 2, 2, 2)}


def set_modes(lib, modes):
    """sets the four kernel-selection modes; returns the previous ones (hand them back in a finally)"""
    return (lib.a3t_gemm_8p_mode(modes[0]), lib.a3t_gemm_pn_mode(modes[1]), lib.a3t_gemm_tt_mode(modes[2]), lib.a3t_gemm_tn3_mode(modes[3]))


def _b(name, seed, M, N, K, ly, dt=BB, **k):
    return build(name, seed, M, N, K, ly, compute=BF16, dt=dt, **k)


def glds_cases():
    """the 128-row direct-to-LDS kernel, every other bf16 route switched off"""
    c, s = [], 5000
    for ly in ("NT", "NN", "TN"):
        s += 10
        c.append(_b(f"glds {ly}", s, 136, 72, 40, ly))
        c.append(_b(f"glds {ly} tails epilogue", s + 1, 200, 136, 72, ly, BF, bias=True, act=ACT_RELU, S="bf16", alpha=0.5, R=True, colsum=True,
                    colsum_scale=0.5))
        c.append(_b(f"glds {ly} 192 columns", s + 2, 72, 192, 64, ly, S="f32", colsum=True, colsum_slots=4))
        c.append(_b(f"glds {ly} one stage", s + 3, 8, 8, 16, ly, batch=768, batch_inner=4, b_bs="shared" if ly == "NT" else "dense"))
        c.append(_b(f"glds {ly} split K", s + 4, 136, 72, 520, ly, BF, acc=ACC_ATOMIC, splitk=3, alpha=-2.0, R=True))
        c.append(_b(f"glds {ly} batch strides bf16 add", s + 5, 72, 136, 24, ly, batch=6, batch_inner=3, a_bs="swap", c_bs="swap", bs_gap=8, acc=ACC_ADD,
                    colsum=True, colsum_scale=0.25))
        c.append(_b(f"glds {ly} dropout", s + 6, 136, 72, 64, ly, drop=(0.5, 99 + s), bias=True))
    for ly, pad in (("NT", 1), ("NN", 0), ("NT", 2), ("NN", 1)):
        s += 10
        c.append(_b(f"glds conv {ly} whole tiles", s, 3 * 56, 72, 3 * 64, ly, taps=3, pad=pad, dil=2, Tseq=56, bias=ly == "NT"))
        c.append(_b(f"glds conv {ly} generic", s + 1, 3 * 7 * 8, 40, 5 * 8, ly, BF, taps=5, pad=pad + 1, dil=1, Tseq=7, S="bf16", alpha=0.5))
    for kshift in (-2, 0, 3, 50, -50):
        s += 1
        c.append(_b(f"glds kshift {kshift}", s, 72, 136, 200, "TN", BF, Tseq=50, kshift=kshift, acc=ACC_ATOMIC, splitk=2))
    c.append(_b("glds fused conv weight gradient", s + 1, 72, 3 * 128, 3 * 56, "TN", BF, taps=3, pad=1, dil=2, Tseq=56, acc=ACC_SOLE, splitk=2, alpha=0.5))
    c.append(_b("glds fused conv weight gradient k5", s + 2, 8, 5 * 128, 4 * 8, "TN", BF, taps=5, pad=4, dil=1, Tseq=8, acc=ACC_ADD))
    c.append(_b("glds sign mask", s + 3, 136, 72, 200, "TN", signmask=True, alpha=2.0, batch=2))
    c.append(_b("glds unaligned view of A", s + 4, 136, 72, 64, "NT", a_ld=65, offs=(1, 0, 0), a_view=True))
    c.append(_b("glds overlapping rows", s + 5, 200, 72, 64, "NT", a_ld=8))
    return c


def g8_cases():
    """mode '8p': the persistent 256 x 256 kernel (NT) and the 256 x 256 token reduction (TN)"""
    s = 6000
    return [_b("8p", s, 264, 136, 128, "NT", bias=True, act=ACT_RELU),
            _b("8p f32 C residual colsum", s + 1, 300, 264, 256, "NT", BF, R=True, alpha=0.5, colsum=True, colsum_scale=-2.0),
            _b("8p strided dropout", s + 2, 520, 72, 128, "NT", a_ld=136, b_ld=144, c_ld=80, offs=(8, 8, 8), drop=(0.5, 31), bias=True),
            _b("8p conv", s + 3, 3 * 50, 72, 3 * 128, "NT", taps=3, pad=1, dil=1, Tseq=50, bias=True, act=ACT_RELU),
            _b("8p conv dilated", s + 4, 3 * 7, 264, 5 * 128, "NT", BF, taps=5, pad=4, dil=2, Tseq=7, R=True),
            _b("8p conv 1-frame utterances", s + 5, 16, 8, 3 * 128, "NT", taps=3, pad=0, dil=4, Tseq=1, colsum=True)]


def tn_cases():
    """modes '8p' (256 x 256 tiles) and 'tn3' (128 x 384 tiles): token reductions into fp32 C"""
    s = 6100
    return [_b("tn store", s, 136, 264, 72, "TN", BF, alpha=0.5),
            _b("tn sole", s + 1, 264, 392, 200, "TN", BF, acc=ACC_SOLE, splitk=2, alpha=-2.0),
            _b("tn atomic strided", s + 2, 72, 136, 136, "TN", BF, a_ld=80, b_ld=144, c_ld=140, offs=(8, 8, 4), acc=ACC_ATOMIC),
            _b("tn K splits and fold", s + 3, 136, 72, 2120, "TN", BF, acc=ACC_SOLE, alpha=0.25),
            _b("tn add", s + 4, 8, 8, 8, "TN", BF, acc=ACC_ADD),
            _b("tn fused conv weight gradient", s + 5, 72, 3 * 128, 3 * 56, "TN", BF, taps=3, pad=1, dil=2, Tseq=56, acc=ACC_SOLE, alpha=0.5),
            _b("tn fused conv weight gradient k5 splits", s + 6, 8, 5 * 128, 2112, "TN", BF, taps=5, pad=2, dil=1, Tseq=66, acc=ACC_SOLE),
            _b("tn fused conv weight gradient short utterances", s + 7, 136, 3 * 256, 8 * 3, "TN", BF, taps=3, pad=2, dil=4, Tseq=3, acc=ACC_STORE)]


def pn_cases():
    """mode 'pn': the 160-row x 384-column panel kernel"""
    s = 6200
    return [_b("pn 384", s, 200, 384, 64, "NT", bias=True, act=ACT_RELU),
            _b("pn narrow f32 C residual mask", s + 1, 330, 136, 128, "NT", BF, R=True, S="bf16", alpha=0.5),
            _b("pn two chunks masked colsum", s + 2, 170, 768, 64, "NT", S="f32", colsum=True, colsum_scale=0.5),
            _b("pn strided dropout", s + 3, 161, 392, 192, "NT", a_ld=200, b_ld=208, c_ld=400, offs=(8, 8, 8), drop=(0.5, 77), bias=True),
            _b("pn conv", s + 4, 3 * 56, 384, 3 * 64, "NT", taps=3, pad=1, dil=1, Tseq=56, bias=True, act=ACT_RELU),
            _b("pn conv dilated", s + 5, 3 * 7, 72, 5 * 64, "NT", BF, taps=5, pad=0, dil=2, Tseq=7, R=True),
            _b("pn conv 1-frame utterances", s + 6, 168, 136, 3 * 128, "NT", taps=3, pad=2, dil=4, Tseq=1, colsum=True, S="bf16")]


def tt_cases():
    """mode 'tt': the streaming kernel (bf16 C, B [k][n])"""
    s = 6300
    return [_b("tt nn", s, 136, 64, 72, "NN", batch=4, batch_inner=2, a_bs="swap"),
            _b("tt nn wide", s + 1, 72, 160, 40, "NN", alpha=0.5, colsum=True, colsum_slots=4),
            _b("tt tn", s + 2, 72, 160, 136, "TN", batch=3, alpha=-2.0),
            _b("tt tn row tiles", s + 3, 648, 64, 72, "TN", acc=ACC_ADD, colsum=True, colsum_scale=0.5),
            _b("tt tn sign mask", s + 4, 136, 96, 200, "TN", signmask=True, alpha=2.0, batch=4, batch_inner=2, b_bs="swap", colsum=True),
            _b("tt two products", s + 5, 136, 64, 72, "NN", second=True, batch=2),
            _b("tt two products colsums", s + 6, 328, 128, 40, "NN", second=True, alpha=0.5, batch=4, batch_inner=2, colsum=True, colsum_slots=4,
               colsum_scale=0.5),
            _b("tt two products wide view", s + 7, 72, 192, 72, "NN", second=True, a2_rs=73)]


def legacy_cases():
    """the register-staged kernel: fp32 operand storage, or bf16 operands outside the direct-to-LDS alignment contract"""
    c, s = [], 6400
    for ly in ("NT", "NN", "TN"):
        for dt in (("f32", "f32", "f32"), ("f32", "bf16", "bf16"), ("bf16", "f32", "f32")):
            s += 1
            c.append(_b(f"legacy {ly} {dt[0]} x {dt[1]}", s, 132 if ly == "TN" else 129, 37 if ly == "NT" else 36, 72, ly, dt, bias=True, act=ACT_RELU, S="bf16", alpha=0.5,
                        R=dt[2] == "f32"))
    c.append(_b("legacy bf16 x bf16, N % 8 != 0", s + 1, 136, 12, 40, "NN", BF, acc=ACC_ATOMIC, splitk=2))
    c.append(_b("legacy bf16 x bf16, M % 8 != 0", s + 2, 132, 36, 50, "TN", BF, Tseq=50, kshift=-1, acc=ACC_SOLE))
    c.append(_b("legacy conv", s + 3, 21, 37, 24, "NT", ("f32", "bf16", "f32"), taps=3, pad=1, dil=2, Tseq=7))
    c.append(_b("legacy conv data gradient", s + 4, 21, 8, 40, "NN", ("bf16", "f32", "f32"), taps=5, pad=2, dil=1, Tseq=7))
    return c


# (mode, cases, prefix of the kernel names they must run on)
def bf16_route_table():
    return [("off", glds_cases(), "gemm_bf16_glds_kernel"), ("8p", g8_cases(), "gemm_bf16_8p_kernel"), ("8p", tn_cases(), "gemm_bf16_8p_tn_kernel"),
            ("tn3", tn_cases(), "gemm_bf16_8p_tn3_kernel"), ("pn", pn_cases(), "gemm_bf16_pn_kernel"), ("tt", tt_cases(), "gemm_bf16_tt_kernel"),
            ("off", legacy_cases(), "gemm_bf16_kernel")]
