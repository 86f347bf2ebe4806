"""float64 reference, error bound, a host restatement of the task walk and the case table for the attention score-gradient kernel
(a3t_attn_bwd_ds, attn_bwd_ds_kernel in csrc/attn_fused.hip), and float64 references of the fused forward's edges.

Used by tests/test_attn_ref_host.py (no GPU), tests/test_gpu_attn_walk.py and tests/test_gpu_attn_edges.py.

Reference (`ref_bwd_ds`).  The kernel's definition, evaluated in float64 on the bf16 / fp32 operands the kernel receives:

    want[b,h,i,j] = |p_ij| rowscale_i scale (keep_ij drop_inv sum_k dctx_ik v_jk - delta_i),   delta_i = sum_k dctx_ik ctx_ik

`scale` is the fp32 value the C entry point receives, `drop_inv` the fp32 quotient 1.f / (1.f - p) the launcher forms.  keep is all
ones (DROP 0), the counter generator's flag of element (bh T + i) T + j mod 2^32 (DROP 1, `ibase` in the kernel), or the sign bit
of probs cleared (DROP 2).  The compact dBD matrix is the inverse legacy skew of dS, element for element (`inverse_skew`).

Bound (`bound_ds`), read off the tile loop of the kernel (the lines between `f32x16 dP = zero16()` and the store of `o`):

1. dP_ij: dk bf16 x bf16 products (exact in fp32) accumulated in fp32 by KS = dk/16 MFMAs: at most dk roundings of partial sums
   that never exceed sum_k |dctx_ik||v_jk|  ->  dk 2^-24 sum_k |dctx_ik||v_jk|.
2. DROP != 0: d = dP * drop_inv, one rounding.
3. delta_i: a chain of dk/2 fp32 FMAs per lane and one addition of the two half rows (lane ^ 32)
   ->  (dk/2 + 1) 2^-24 sum_k |dctx_ik||ctx_ik|.
4. in_rsc = rowscale * scale; p * rsc; d - dl; the product of the two: four roundings of values bounded by the magnitude below.
5. io_pack2: ONE round-to-nearest-even to bf16.

1.-4. together stay below (dk + 8) 2^-24 M with M = |p| rowscale scale (drop_inv sum_k |dctx||v| + sum_k |dctx||ctx|); the bound
takes (dk + 8) 2^-23 M, twice that, for second-order terms and because an MFMA's internal order of additions is not documented.
5.: a bf16 value has 8 significant bits, so rounding x moves it by at most half a unit in its last place,
hulp(x) = 2^(floor(log2 |x|) - 8), which lies between 2^-9 |x| (x just below a power of two) and 2^-8 |x| (x a power of two).
2^-9 |want| alone is NOT a bound of a correct rounding (1 + 2^-8 rounds to 1 or to 1 + 2^-7, either way 2^-8 off); the term here
is hulp(want), the smallest that is.  (x is the fp32 value, not want: when the two fall on different sides of a rounding boundary
the result is off by the distance of want to that boundary, which the fp32 term covers, plus the half-ulp of the finer side.)
Below 2^-126 the bf16 grid has the subnormal spacing 2^-133, which is added there.

    bound = hulp(want) + (dk + 8) 2^-23 M + (2^-133 where |want| < 2^-126)

tests/test_attn_ref_host.py checks this derivation without a GPU: two fp32 emulations of the arithmetic above (sequential and
pairwise dot products) stay inside the bound after the bf16 rounding, and inside HALF of the fp32 term before it.

Walk (`walk`).  The launcher starts grid = min(2 CUs, ntasks) workgroups, ntasks = B H NQB NKC with NQB = ceil(T/128) query blocks
and NKC = ceil(ceil(T/32)/5) strips of up to five 32-key tiles; the strip index is the fastest digit of a task, then the query
block, then (b, h).  Workgroup `blockIdx.x` takes range index vb = xcd_contiguous(blockIdx.x, grid) and walks the tasks
vb tper .. min((vb + 1) tper, ntasks) - 1 with tper = ceil(ntasks / grid).  Because the strips of a query block are consecutive
tasks, a range only starts inside a query block, or crosses a (b, h) boundary, when tper is not a multiple of NKC resp. NQB NKC
does not divide into it: the cases named `cross_*` below are chosen that way; a table with tper = NKC everywhere would only ever
meet the `same-block` transition.
"""
import collections
import math
import zlib

import numpy as np
import torch

import stepkernel_ref as SK

F64 = torch.float64
KT = 5                     # key tiles per strip
U23 = 2.0 ** -23
DKS = (32, 64, 96, 128, 192)


# ----------------------------------------------------------------------------------------------------------------------
# a. the reference and its bound
# ----------------------------------------------------------------------------------------------------------------------
Ds = collections.namedtuple("Ds", "ref mag keep dk")


def f32(x):
    return float(np.float32(x))


def heads(x, B, H, T, dk):
    """[B*T][>= H*dk] rows (head h at columns h*dk ..) -> [B][H][T][dk] in float64."""
    return x[:, :H * dk].to(F64).reshape(B, T, H, dk).transpose(1, 2)


def keep_of(probs_bits, drop, mode):
    """The keep flags [B][H][T][T] (bool) of a launch: see the module docstring."""
    B, H, T, _ = probs_bits.shape
    if mode == 0:
        return torch.ones(B, H, T, T, dtype=torch.bool, device=probs_bits.device)
    if mode == 2:
        return probs_bits.contiguous().view(torch.int16) >= 0
    n = B * H * T * T
    k = SK.keep(drop[1], np.arange(n, dtype=np.int64), drop[0])
    return torch.from_numpy(k).view(B, H, T, T).to(probs_bits.device)


def ref_bwd_ds(dctx, ctx, v, probs_bits, rowscale, scale, drop, mode):
    """dctx, ctx: [B*T][H*dk] bf16; v: [B*T][H*dk] bf16 (any row stride); probs_bits: [B][H][T][T] bf16 as stored (sign-tagged for
    mode 2); rowscale: [B][H][T] fp32; drop = (p, key); mode = the kernel's DROP.  -> Ds(ref, mag, keep, dk), float64 on the
    operands' device."""
    B, H, T, _ = probs_bits.shape
    dk = dctx.shape[1] // H
    dc, cx, vv = heads(dctx, B, H, T, dk), heads(ctx, B, H, T, dk), heads(v, B, H, T, dk)
    keep = keep_of(probs_bits, drop, mode)
    dinv = float(SK.drop_inv(drop[0])) if mode else 1.0
    pn = probs_bits.abs().to(F64) * rowscale.to(F64)[..., None] * f32(scale)
    delta = (dc * cx).sum(-1)
    ref = pn * (keep.to(F64) * dinv * (dc @ vv.transpose(-1, -2)) - delta[..., None])
    mag = pn * (dinv * (dc.abs() @ vv.abs().transpose(-1, -2)) + (dc.abs() * cx.abs()).sum(-1)[..., None])
    return Ds(ref, mag, keep, dk)


def hulp_bf16(x):
    """Half a unit in the last place of a bf16 value of x's magnitude: 2^(floor(log2 |x|) - 8); 0 for x = 0."""
    _, e = torch.frexp(x.abs())                      # |x| = m 2^e with m in [0.5, 1)
    h = torch.ldexp(torch.ones_like(x), e - 9)
    return torch.where(x == 0, torch.zeros_like(x), h)


def fp32_term(o):
    return (o.dk + 8) * U23 * o.mag


def bound_ds(o):
    """The tolerance of dS per element: see the module docstring."""
    sub = (o.ref.abs() < 2.0 ** -126).to(F64) * 2.0 ** -133
    return hulp_bf16(o.ref) + fp32_term(o) + sub


def inverse_skew(ds):
    """The compact dBD matrix [..][T][T] of a dS [..][T][T], element for element: keys j <= i of query i go to row i from column
    T-1-i, keys j >= i+2 to row i+1 from column 0 (the adjoint of attention.py:145-165; key i+1 reads the padding column and has
    no gradient).  Row 0, columns 0..T-2 stay zero."""
    T = ds.shape[-1]
    out = torch.zeros(ds.shape[:-2] + (T + 1, T), dtype=ds.dtype, device=ds.device)
    ii = torch.arange(T, device=ds.device)[:, None].expand(T, T)
    jj = torch.arange(T, device=ds.device)[None, :].expand(T, T)
    lo, up = jj <= ii, jj >= ii + 2
    out[..., ii[lo], (T - 1 - ii + jj)[lo]] = ds[..., ii[lo], jj[lo]]
    out[..., (ii + 1)[up], (jj - ii - 2)[up]] = ds[..., ii[up], jj[up]]
    return out[..., :T, :].contiguous()


def emulate_fp32(dctx, ctx, v, probs_bits, rowscale, scale, drop, mode, pairwise):
    """The kernel's arithmetic in fp32 with a stated order of additions: dot products sequential over k (pairwise=False) or by
    recursive halving (True); delta as the kernel forms it (two half rows, then one addition).  -> (fp32 value before the store,
    the bf16 value stored), both float64."""
    B, H, T, _ = probs_bits.shape
    dk = dctx.shape[1] // H
    t = lambda x: x[:, :H * dk].to(torch.float32).reshape(B, T, H, dk).transpose(1, 2).contiguous()
    dc, cx, vv = t(dctx), t(ctx), t(v)

    def dot(prod):                                   # prod(k) -> the products of column k; summed over k in fp32
        if pairwise:
            def rec(k0, k1):
                if k1 - k0 == 1:
                    return prod(k0)
                m = (k0 + k1) // 2
                return rec(k0, m) + rec(m, k1)
            return rec(0, dk)
        acc = prod(0)
        for k in range(1, dk):
            acc = acc + prod(k)
        return acc

    dP = dot(lambda k: dc[..., :, None, k] * vv[..., None, :, k])        # products of bf16 pairs are exact in fp32
    half = dk // 2
    if pairwise:
        dl = dot(lambda k: dc[..., k] * cx[..., k])
    else:
        lo = dc[..., 0] * cx[..., 0]
        for k in range(1, half):
            lo = lo + dc[..., k] * cx[..., k]
        hi = dc[..., half] * cx[..., half]
        for k in range(half + 1, dk):
            hi = hi + dc[..., k] * cx[..., k]
        dl = lo + hi
    keep = keep_of(probs_bits, drop, mode)
    if mode:
        dP = torch.where(keep, dP * torch.tensor(SK.drop_inv(drop[0])), torch.zeros_like(dP))
    rsc = rowscale.to(torch.float32) * torch.tensor(np.float32(scale))
    x = probs_bits.abs().to(torch.float32) * rsc[..., None] * (dP - dl[..., None])
    return x.to(F64), x.to(torch.bfloat16).to(F64)


# ----------------------------------------------------------------------------------------------------------------------
# b. the walk, restated
# ----------------------------------------------------------------------------------------------------------------------
Geometry = collections.namedtuple("Geometry", "NS NKC NQB ntasks grid tper")
Task = collections.namedtuple("Task", "index bh b h qb kc sa nt J0 J1 facts")
Group = collections.namedtuple("Group", "block vb tasks transitions facts")
Walk = collections.namedtuple("Walk", "geometry groups")


def _cdiv(a, b):
    return -(-a // b)


def geometry(B, H, T, cus):
    NS, NQB = _cdiv(T, 32), _cdiv(T, 128)
    NKC = _cdiv(NS, KT)
    ntasks = B * H * NQB * NKC
    grid = min(2 * cus, ntasks)
    return Geometry(NS, NKC, NQB, ntasks, grid, _cdiv(ntasks, grid))


def xcd_contiguous(wi, nwg):
    """mfma_kit.h: workgroup ids are dealt round-robin over 8 XCDs; the workgroups of one XCD take neighbouring range indices."""
    q, r, xcd = nwg >> 3, nwg & 7, wi & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (wi >> 3)


def decode(task, H, T):
    """A3T_DS_DECODE."""
    NS, NQB = _cdiv(T, 32), _cdiv(T, 128)
    NKC = _cdiv(NS, KT)
    kc, t2 = task % NKC, task // NKC
    qb, bh = t2 % NQB, t2 // NQB
    sa = kc * KT
    sb = min(sa + KT, NS)
    facts = {f"nt{sb - sa}"}
    if T % 32 and sb == NS:
        facts.add("partial-tile")
    if any(128 * qb + 32 * w >= T for w in range(4)):
        facts.add("wave-past-T")
    return Task(task, bh, bh // H, bh % H, qb, kc, sa, sb - sa, 32 * sa, min(32 * sb, T), frozenset(facts))


def transition(c, n):
    """The labels of the step from task c to task n inside one workgroup."""
    lab = set()
    if n.bh == c.bh and n.qb == c.qb:
        lab.add("same-block")                        # fetch_rows is false
    elif n.bh == c.bh:
        lab.add("new-block")
    elif n.b == c.b:
        lab.add("new-head")
    else:
        lab.add("new-batch")
    if c.nt == 1:
        lab.add("nt1->ntN" if n.nt > 1 else "nt1->nt1")
    return frozenset(lab)


def walk(B, H, T, cus):
    """-> Walk(geometry, groups): one Group per workgroup (blockIdx.x order) with its range index, its tasks, the labels of each
    transition between consecutive tasks and the facts `idle` / `short-last`."""
    g = geometry(B, H, T, cus)
    groups = []
    for wi in range(g.grid):
        vb = xcd_contiguous(wi, g.grid)
        first = vb * g.tper
        tend = min(first + g.tper, g.ntasks)
        tasks = [decode(t, H, T) for t in range(first, tend)]
        facts = set()
        if not tasks:
            facts.add("idle")
        elif len(tasks) < g.tper:
            facts.add("short-last")
        groups.append(Group(wi, vb, tasks, [transition(a, b) for a, b in zip(tasks, tasks[1:])], frozenset(facts)))
    return Walk(g, groups)


def labels(w):
    out = set()
    for gr in w.groups:
        out |= gr.facts
        for t in gr.tasks:
            out |= t.facts
        for tr in gr.transitions:
            out |= tr
    return out


def transition_labels(w):
    out = set()
    for gr in w.groups:
        for tr in gr.transitions:
            out |= tr
    return out


def locate(w, bh, i, j):
    """Which workgroup wrote dS[bh][i][j], and through which transition it came to that task: the text of an assertion message."""
    g = w.geometry
    task = (bh * g.NQB + i // 128) * g.NKC + (j // 32) // KT
    for gr in w.groups:
        for n, t in enumerate(gr.tasks):
            if t.index == task:
                how = "its first task" if n == 0 else "after " + "+".join(sorted(gr.transitions[n - 1]))
                return (f"task {task} (bh {bh}, query block {t.qb}, strip {t.kc}, nt {t.nt}, tile {(j // 32) % KT} of it, wave {(i % 128) // 32}), "
                        f"task {n + 1} of {len(gr.tasks)} of workgroup {gr.block} (range {gr.vb}), {how}")
    return f"task {task}: in no workgroup's range"


REQUIRED_LABELS = frozenset({
    "same-block", "new-block", "new-head", "new-batch", "nt1->ntN", "nt1->nt1", "idle", "short-last",
    "nt1", "nt2", "nt3", "nt4", "nt5", "partial-tile", "wave-past-T"})


# ----------------------------------------------------------------------------------------------------------------------
# c. the case table
# ----------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name B H T dk mode dbd tper")        # dbd: "bm" batch-major, "hm" head-major, None
DROP = (0.2, 0x5151)


def _split(bh):
    """B, H with B H = bh: the smallest H in 2..8 that divides (so (b, h) boundaries are of both kinds), else one head."""
    for H in range(2, 9):
        if bh % H == 0 and bh // H >= 3:
            return bh // H, H
    return bh, 1


def _fit(T, H, tper, cus, ragged_end):
    """The smallest B >= 3 whose walk has `tper` tasks per workgroup (and, if ragged_end, a short last workgroup)."""
    for B in range(3, 100000):
        g = geometry(B, H, T, cus)
        if g.tper > tper:
            break
        if g.tper == tper and g.grid == 2 * cus and (not ragged_end or g.ntasks % tper):
            return B
    raise AssertionError((T, H, tper, cus))


def cases(cus):
    """The table for a device of `cus` compute units (G = 2 cus workgroups).  Every case has B >= 3: batch row 1 is ragged and
    batch row 2 fully masked (make_operands)."""
    G = 2 * cus
    out = []

    def add(name, B, H, T, dk, tper, modes=(0,), dbd="bm"):
        for m in modes:
            c = Case(name + ("" if m == 0 or name == "production" else f"_drop{m}"), B, H, T, dk, m, dbd, tper)
            assert geometry(B, H, T, cus).tper == tper, c
            out.append(c)

    # one tile per task, two tasks per workgroup: every transition changes (b, h) and keeps q0; an odd H so that both kinds occur
    bh = G + 8
    H = next((h for h in (3, 5, 7, 9, 11, 13, 17, 19) if bh % h == 0), 1)
    add("one_tile", bh // H, H, 32, 32, 2)
    # strips (5, 1), two tasks per workgroup = one query block each
    B, H = _split(_cdiv(G + 1, 4))
    for n, dk in enumerate(DKS):
        add(f"strip_5_1_dk{dk}", B, H, 168, dk, 2, modes=(0, 1, 2) if dk == 64 else (0,), dbd=("bm", "hm", None)[n % 3])
    for n, (T, tasks) in enumerate(((200, 4), (232, 4), (264, 6))):
        B, H = _split(_cdiv(G + 1, tasks))
        add(f"strip_5_{2 + n}", B, H, T, 64, 2, dbd=("hm", None, "bm")[n])
    # strips (5, 5, 1), three tasks per workgroup = one query block each
    B, H = _split(_cdiv(2 * G + 1, 9))
    add("tper3_dk64", B, H, 328, 64, 3, dbd=None)
    add("tper3_dk192", B, H, 328, 192, 3, modes=(0, 1, 2), dbd="hm")
    # ranges that start inside a query block and cross query blocks, heads and batch rows (see the module docstring):
    # four tasks per (b, h) walked in threes, nine walked in twos; the last workgroup is short
    B = _fit(168, 2, 3, cus, True)
    for n, dk in enumerate(DKS):
        add(f"cross_5_1_dk{dk}", B, 2, 168, dk, 3, modes=(0, 1, 2) if dk == 64 else (0,), dbd=("hm", "bm", None)[n % 3])
    B = _fit(328, 3, 2, cus, True)
    add("cross_5_5_1_dk64", B, 3, 328, 64, 2, dbd="bm")
    add("cross_5_5_1_dk192", B, 3, 328, 192, 2, modes=(0, 1, 2), dbd=None)
    # the training step's form of the launch: sign-tagged probabilities, no dBD, T zeros in front of every block of dS
    add("production", _fit(168, 2, 3, cus, True), 2, 168, 192, 3, modes=(2,), dbd=None)
    return tuple(out)


CASE_NAMES = tuple(c.name for c in cases(256))


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def lengths_of(B, T):
    """Valid keys per batch row: row 1 ragged (not a multiple of 8), row 2 fully masked."""
    L = [T] * B
    if B > 1:
        L[1] = max(1, (5 * T) // 8 - 3)
    if B > 2:
        L[2] = 0
    return L


def make_operands(B, H, T, dk, mode, seed, lengths=None):
    """Synthetic operands of one launch (CPU tensors), shaped like a training step's: scores ~ N(0, 1.5^2), probs = bf16(exp(s -
    row maximum)) with exact zeros in the masked key columns, rowscale = 1 / row sum in fp32 (0 for a row without a valid key), v and
    dctx standard normal in bf16, ctx = bf16(dropped, normalised probs @ v) so that delta cancels against dP as it does in
    training; mode 2 sets the sign bit on a Bernoulli(p) mask, mode 1 takes the counter generator's mask.
    -> dict(dctx, ctx [B*T][d] bf16, qkv [B*T][3d] bf16 with NaN in the q and k columns, probs [B][H][T][T] bf16, rowscale
    [B][H][T] fp32, scale, drop, lengths)."""
    g = torch.Generator().manual_seed(seed)
    d = H * dk
    lengths = lengths_of(B, T) if lengths is None else lengths
    valid = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]                    # [B][T]
    s = torch.randn(B, H, T, T, generator=g) * 1.5
    s = s.masked_fill(~valid[:, None, None, :], -float("inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))            # exact zeros in masked columns
    probs = e.to(torch.bfloat16)
    rsum = e.sum(-1)
    rowscale = torch.where(rsum > 0, 1.0 / rsum, torch.zeros_like(rsum)).to(torch.float32)
    v = torch.randn(B * T, d, generator=g).to(torch.bfloat16)
    dctx = torch.randn(B * T, d, generator=g).to(torch.bfloat16)
    drop = DROP if mode else (0.0, 0)
    if mode == 2:
        dropped = torch.rand(B, H, T, T, generator=g) < drop[0]
        probs = torch.where(dropped, -probs, probs)                                      # (-0.0 where a zero is tagged)
    keep = keep_of(probs, drop, mode)
    dinv = float(SK.drop_inv(drop[0])) if mode else 1.0
    pd = probs.abs().float() * rowscale[..., None] * keep * dinv
    ctx = (pd @ v.float().view(B, T, H, dk).transpose(1, 2)).transpose(1, 2).reshape(B * T, d).to(torch.bfloat16)
    qkv = torch.full((B * T, 3 * d), float("nan"), dtype=torch.bfloat16)
    qkv[:, 2 * d:] = v
    return dict(dctx=dctx, ctx=ctx, qkv=qkv, probs=probs.contiguous(), rowscale=rowscale.contiguous(), scale=1.0 / math.sqrt(dk),
                drop=drop, lengths=lengths)


def case_operands(case):
    return make_operands(case.B, case.H, case.T, case.dk, case.mode, seed_of(case.name))


# ----------------------------------------------------------------------------------------------------------------------
# d. the fused forward (a3t_attn_fwd / a3t_attn_fwd_train), for tests/test_gpu_attn_edges.py
# ----------------------------------------------------------------------------------------------------------------------
def rel_shift_legacy(x):
    """LegacyRelPositionMultiHeadedAttention.rel_shift (attention.py:145-165): a zero column in front, the rows re-cut."""
    B, H, T1, T2 = x.shape
    xp = torch.cat([x.new_zeros(B, H, T1, 1), x], dim=-1).view(B, H, T2 + 1, T1)
    return xp[:, :, 1:].reshape(B, H, T1, T2)


def ref_fwd(qkv, qu, qv, P, keymask, B, H, T, dk, keep=None, dinv=1.0):
    """The legacy rel-pos attention in float64 on the bf16 operands (the formula of _exact in tests/test_gpu_attn_fused.py), on the
    operands' device: qkv [B*T][3d], qu / qv = q + pos_bias_u / v [B*T][d], P = linear_pos(pos) [T][d], keymask [B][T].
    -> ctx [B*T][d] (from keep * dinv * softmax when a dropout mask is given), softmax [B][H][T][T] (0 in masked columns and in
    rows without a valid key), lse [B][H][T] (-inf in such rows)."""
    d = H * dk
    k, v = heads(qkv[:, d:2 * d], B, H, T, dk), heads(qkv[:, 2 * d:], B, H, T, dk)
    p = P.to(F64).view(T, H, dk).transpose(0, 1)[None]
    ac = heads(qu, B, H, T, dk) @ k.transpose(-1, -2)
    bd = rel_shift_legacy(heads(qv, B, H, T, dk) @ p.transpose(-1, -2))
    sc = (ac + bd) / math.sqrt(dk)
    m = keymask.bool()[:, None, None, :]
    sc = sc.masked_fill(~m, -float("inf"))
    lse = torch.logsumexp(sc, dim=-1)
    pr = torch.nan_to_num(torch.softmax(sc, dim=-1).masked_fill(~m, 0.0), nan=0.0)
    pd = pr if keep is None else pr * keep.to(F64) * dinv
    ctx = (pd @ v).transpose(1, 2).reshape(B * T, d)
    return ctx, pr, lse


LADDER_T = (8, 16, 24, 32, 64, 96, 120, 128)
LADDER_DK = (32, 192)
