"""The ParallelWaveGAN kernels one by one against the float64 references of tests/pwg_ref.py: the fused fp32 residual block
(a3t_pwg_block, a3t_pwg_block_ragged) at tile edges and with NaN padding, the persistent multi-tile walk of pwg_stage_kernel and
pwg_f16_kernel (more tiles than the device has CUs) against float64 and against the same tiles computed one per workgroup, the
layer-path helpers (a3t_pwg_gate, a3t_pwg_res_skip, a3t_pwg_upsample, a3t_replicate_pad, a3t_zero_tail, a3t_reflect_pad_rows and
their ragged forms), and what the block's entry points refuse.  Bounds: the docstring of pwg_ref.py."""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pwg_f16_ref as R
import pwg_ref as P
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
GUARD = 1024                  # floats in front of and behind every guarded buffer (4 KiB: the views stay 16-byte aligned)
GUARD_VALUE = 31337.0
EINVAL = -22
LAUNCHES = collections.Counter()
WALKED = {"fp32": 0, "f16": 0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlaunches per kernel instantiation:", dict(sorted(LAUNCHES.items())))
    print("most tiles one workgroup walked:", WALKED)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded:
    """A device buffer between two bands of GUARD_VALUE; .t is the tensor in the middle."""

    def __init__(self, src=None, shape=None, fill=None, dtype=torch.float32):
        shape = tuple(src.shape) if src is not None else tuple(shape)
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if src is not None:
            self.t.copy_(src)
        elif fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == GUARD_VALUE).all()) and bool((self.buf[-GUARD:] == GUARD_VALUE).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _operands():
    """The packed operands of the block under test: (wt0, b0, wt1, b1) on the host and on the device, and the raw parameters."""
    from a3t_amd.vocoder import _pack_pwg_block
    cw, cb, aw, ow, ob = P.block_params()
    host = (*_pack_pwg_block(cw, cb, aw, ow), ob)
    return host, tuple(t.to(DEV) for t in host), (cw, cb, aw, ow, ob)


def _tiles_dev(tiles):
    return torch.from_numpy(np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 4)).to(DEV)


def _block(x, cu, sk, B, Tw, dil, tiles=None):
    """ops.pwg_block on guarded copies of x and skips ([B][Tw][64] device tensors; cu is shared) -> (x_out, skips_out) [B][Tw][64]
    on the device.  Guard bands, cu and the weights are checked here."""
    from a3t_amd import ops
    _, dev, _ = _operands()
    keep = [t.clone() for t in dev]
    gx, gg, gs = Guarded(x.reshape(B * Tw, 64)), Guarded(shape=(B * Tw, 64), fill=float("nan")), Guarded(sk.reshape(B * Tw, 64))
    td = None if tiles is None else _tiles_dev(tiles)
    ops.pwg_block(gx.t, cu.view(B * Tw, 80), dev[0], dev[1], dev[2], dev[3], gg.t, gs.t, B, Tw, dil, td)
    torch.cuda.synchronize()
    ntiles = B * -(-Tw // 256) if tiles is None else len(tiles)
    LAUNCHES[f"pwg_stage_kernel<0|1, {'true' if tiles is not None else 'false'}>"] += 1
    WALKED["fp32"] = max(WALKED["fp32"], max(len(g) for g in P.walk(ntiles, _cus())))
    assert gx.intact() and gg.intact() and gs.intact(), "a guard band was written"
    assert all(_same_bits(a, b) for a, b in zip(keep, dev)), "the block wrote to its weights"
    return gx.t.view(B, Tw, 64), gs.t.view(B, Tw, 64)


def _reference(case):
    """dict: the case's inputs, the float64 block and the per-column allowances."""
    host, _, _ = _operands()
    x, cu, sk = P.case_inputs(case)
    r64 = P.block_ref(x, cu, sk, *host, case.dil, case.W)
    r32 = P.block_ref(x, cu, sk, *host, case.dil, case.W, dtype=torch.float32)
    ax, as_, Fx, Fs = P.allowance(r64[:2], r32[:2], r64[2], case.W)
    return dict(x=x, cu=cu, sk=sk, x64=r64[0], s64=r64[1], ax=ax, as_=as_, Fx=Fx, Fs=Fs)


_small_reference = functools.lru_cache(maxsize=None)(_reference)


def _against_float64(case, ref, xo, so, what):
    """x_out and skips within the allowance in front of W_b, bit-identical to what they held behind it."""
    xo, so = xo.cpu(), so.cpu()
    m = P.valid_mask(case.B, case.Tw, case.W)
    ex = ((xo.double() - ref["x64"]).abs() / ref["ax"])[m]
    es = ((so.double() - ref["s64"]).abs() / ref["as_"])[m]
    print(f"{what} {case.name}: worst error / allowance x_out {float(ex.max()):.3f} skips {float(es.max()):.3f} "
          f"(F {ref['Fx']:.2e} / {ref['Fs']:.2e}, allowance {float(ref['ax'].max()):.2e} / {float(ref['as_'].max()):.2e})")
    assert torch.isfinite(xo[m]).all() and torch.isfinite(so[m]).all()
    assert float(ex.max()) <= 1.0 and float(es.max()) <= 1.0
    assert _same_bits(xo[~m], ref["x"][~m]) and _same_bits(so[~m], ref["sk"][~m]), "rows behind W_b changed"


def _on_device(ref):
    x, cu, sk = (ref[k].to(DEV) for k in ("x", "cu", "sk"))
    return x, cu, sk, cu.clone()


def _row_alone(case, x, cu, sk, b):
    """The dense launch of row b alone."""
    n = case.W[b]
    return _block(x[b:b + 1, :n].contiguous(), cu[b:b + 1, :n].contiguous(), sk[b:b + 1, :n].contiguous(), 1, n, case.dil)


# ------------------------------------------------------------------------------------------ 1. one fp32 block against float64
@pytest.mark.parametrize("case", P.BLOCK_CASES, ids=lambda c: c.name)
def test_block_against_float64(case):
    """ops.pwg_block over the block cases (a dense case without and with a tile list of equal lengths, a ragged one with its
    list): inside the allowance in front of W_b, the padding's bit patterns (NaN, sentinel) kept, guard bands, cu and weights
    untouched."""
    ref = _small_reference(case)
    x, cu, sk, cu0 = _on_device(ref)
    for tiles in ([P.tile_list(case.W)] if case.ragged else [None, P.tile_list(case.W)]):
        xo, so = _block(x, cu, sk, case.B, case.Tw, case.dil, tiles)
        _against_float64(case, ref, xo, so, "block" + ("" if tiles is None else "+tiles"))
        assert _same_bits(cu, cu0)


# ----------------------------------------------------------------------------------------------- 2. bit-for-bit properties
@pytest.mark.parametrize("case", [c for c in P.BLOCK_CASES if c.ragged], ids=lambda c: c.name)
def test_ragged_row_equals_the_dense_launch_of_the_row_alone(case):
    ref = _small_reference(case)
    x, cu, sk, _ = _on_device(ref)
    xo, so = _block(x, cu, sk, case.B, case.Tw, case.dil, P.tile_list(case.W))
    for b, n in enumerate(case.W):
        xa, sa = _row_alone(case, x, cu, sk, b)
        assert _same_bits(xo[b, :n], xa[0]) and _same_bits(so[b, :n], sa[0]), b


@pytest.mark.parametrize("case", P.BLOCK_CASES, ids=lambda c: c.name)
def test_shuffled_tile_list_gives_the_bits_of_the_ordered_one(case):
    ref = _small_reference(case)
    x, cu, sk, _ = _on_device(ref)
    tiles = P.tile_list(case.W)
    xo, so = _block(x, cu, sk, case.B, case.Tw, case.dil, tiles)
    xs, ss = _block(x, cu, sk, case.B, case.Tw, case.dil, tiles[np.random.RandomState(5).permutation(len(tiles))])
    assert _same_bits(xo, xs) and _same_bits(so, ss)


@pytest.mark.parametrize("case", [c for c in P.BLOCK_CASES if not c.ragged], ids=lambda c: c.name)
def test_equal_lengths_give_the_bits_of_the_dense_launch(case):
    ref = _small_reference(case)
    x, cu, sk, _ = _on_device(ref)
    xo, so = _block(x, cu, sk, case.B, case.Tw, case.dil)
    xt, st = _block(x, cu, sk, case.B, case.Tw, case.dil, P.tile_list(case.W))
    assert _same_bits(xo, xt) and _same_bits(so, st)


# ------------------------------------------------------------------------------------------------------------ 3. the walk
def _pieces(tiles, cus):
    return [tiles[i:i + cus] for i in range(0, len(tiles), cus)]


@pytest.mark.parametrize("which", range(4), ids=["dense_d1", "dense_d512", "ragged_d1", "ragged_d512"])
def test_walk_against_float64_and_against_one_tile_per_workgroup(which):
    """More tiles than CUs: every workgroup of pwg_stage_kernel walks two or three tiles (pwg_ref.walk_dense / walk_ragged of
    this device's CU count).  The launch against float64, and bit for bit against the same tiles computed one per workgroup:
    the list cut into pieces of at most `cus` entries, each piece on a fresh copy of x and skips (the block is in place and
    stage 0 reads x[t +- dil] of other tiles), compared over that piece's tiles.  The ragged walk also against the shuffled list
    and against its longest and its shortest row alone."""
    cus = _cus()
    case = P.walk_cases(cus)[which]
    tiles = P.tile_list(case.W)
    assert len(tiles) > 2 * cus and P.device_bytes(case) < 512e6
    ref = _reference(case)
    x, cu, sk, cu0 = _on_device(ref)
    xo, so = _block(x, cu, sk, case.B, case.Tw, case.dil, tiles if case.ragged else None)
    _against_float64(case, ref, xo, so, "walk")
    assert _same_bits(cu, cu0)
    xf, sf = xo.reshape(-1, 64), so.reshape(-1, 64)
    for piece in _pieces(tiles, cus):
        xp, sp = _block(x, cu, sk, case.B, case.Tw, case.dil, piece)
        idx = P.tile_samples(piece, case.Tw).to(DEV)
        assert _same_bits(xf[idx], xp.reshape(-1, 64)[idx]) and _same_bits(sf[idx], sp.reshape(-1, 64)[idx])
    if case.ragged:
        xs, ss = _block(x, cu, sk, case.B, case.Tw, case.dil, tiles[np.random.RandomState(6).permutation(len(tiles))])
        assert _same_bits(xo, xs) and _same_bits(so, ss)
        for b in (2, 3):
            xa, sa = _row_alone(case, x, cu, sk, b)
            assert _same_bits(xo[b, :case.W[b]], xa[0]) and _same_bits(so[b, :case.W[b]], sa[0]), b


def _rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt(np.mean(a * a)))


@pytest.mark.parametrize("which", [1, 2], ids=["dense_d512", "ragged_d1"])
def test_walk_f16_against_the_restatement_and_against_one_tile_per_workgroup(which):
    """a3t_pwg_block_f16 over a walk case.  The criterion of test_gpu_vocoder_f16.py's one-block test, per row: RMS(kernel -
    restatement with fp16 rounding) <= 0.1 x RMS(that restatement - the fp32 one); rows behind W_b keep what they held; and the
    same tiles one per workgroup give the same bits."""
    from a3t_amd import ops
    from a3t_amd.vocoder import pack_pwg_block_f16
    cus = _cus()
    case = P.walk_cases(cus)[which]
    tiles = P.tile_list(case.W)
    _, _, (cw, cb, aw, ow, ob) = _operands()
    p = {P.PWG_BLOCK + k: v for k, v in zip(("conv.weight", "conv.bias", "conv1x1_aux.weight", "conv1x1_out.weight",
                                             "conv1x1_out.bias"), (cw, cb, aw, ow, ob))}
    w0h, b0, w1h = (t.to(DEV) for t in pack_pwg_block_f16(cw, cb, aw, ow))
    b1 = ob.to(DEV)
    x, cu, sk = P.case_inputs(case)
    B, Tw, n = case.B, case.Tw, case.B * case.Tw
    xd, skd = x.to(DEV).view(n, 64), sk.to(DEV).view(n, 64)
    cu16 = torch.empty(n, 80, dtype=torch.float16, device=DEV)
    ops.cast_f16_sat(cu.to(DEV).view(n, 80), cu16)

    def run(tl):
        gx, gs = Guarded(shape=(n, 64), fill=777.0), Guarded(skd)
        ops.pwg_block_f16(xd, gx.t, cu16, w0h, b0, w1h, b1, gs.t, None if tl is None else _tiles_dev(tl), B, Tw, case.dil)
        torch.cuda.synchronize()
        LAUNCHES[f"pwg_f16_kernel<{'true' if tl is not None else 'false'}>"] += 1
        WALKED["f16"] = max(WALKED["f16"], max(len(g) for g in P.walk(len(tiles) if tl is None else len(tl), cus)))
        assert gx.intact() and gs.intact()
        return gx.t, gs.t

    xo, so = run(tiles if case.ragged else None)
    assert _same_bits(xd, x.to(DEV).view(n, 64))
    for piece in _pieces(tiles, cus):
        xp, sp = run(piece)
        idx = P.tile_samples(piece, Tw).to(DEV)
        assert _same_bits(xo[idx], xp[idx]) and _same_bits(so[idx], sp[idx])
    xo, so = xo.cpu().view(B, Tw, 64), so.cpu().view(B, Tw, 64)
    cfg = O.PWGConfig()
    for b, nb in enumerate(case.W):
        out = {}
        for name, dt in (("f16", torch.float16), ("f32", None)):
            rnd = R.rounder(dt)
            with torch.no_grad():
                xr, s = R.block(p, P.PWG_BLOCK, x[b, :nb].t()[None], rnd(cu[b, :nb].t()[None]), case.dil, cfg, rnd)
            out[name] = (xr[0].t().numpy(), (sk[b, :nb] + s[0].t()).numpy())
        for what, got, i in (("x_out", xo[b, :nb].numpy(), 0), ("skips", so[b, :nb].numpy(), 1)):
            assert np.isfinite(got).all()
            res, rounding = _rms(got - out["f16"][i]), _rms(out["f16"][i] - out["f32"][i])
            print(f"f16 walk {case.name} row {b} ({nb} samples) {what}: RMS(kernel - restatement) {res:.3e}, "
                  f"RMS(restatement - fp32 restatement) {rounding:.3e}, ratio {res / rounding:.4f}")
            assert res <= 0.1 * rounding, (what, b, res, rounding)
        assert (xo[b, nb:] == 777.0).all() and _same_bits(so[b, nb:], sk[b, nb:])


# ------------------------------------------------------------------------------------------------- 4. layer-path kernels
TRIP = 16390          # T * 64 = 2^20 + 384: one grid-stride trip of 4096 x 256 threads and a ragged remainder


@pytest.mark.parametrize("T", [1, TRIP])
def test_pwg_gate_against_float64(T):
    from a3t_amd import ops
    g = torch.Generator().manual_seed(11)
    y, c = torch.randn(T, 128, generator=g) * 2.0, torch.randn(T, 128, generator=g) * 1.5
    ref, allow = P.gate_ref(y, c)
    out = Guarded(shape=(T, 64), fill=float("nan"))
    ops.pwg_gate(y.to(DEV), c.to(DEV), out.t)
    torch.cuda.synchronize()
    ratio = float(((out.t.cpu().double() - ref).abs() / allow).max())
    print(f"pwg_gate T={T}: worst error / allowance {ratio:.3f}")
    assert out.intact() and ratio <= 1.0


@pytest.mark.parametrize("T", [1, TRIP])
def test_pwg_res_skip_bit_for_bit(T):
    from a3t_amd import ops
    g = torch.Generator().manual_seed(12)
    o, x, sk = torch.randn(T, 128, generator=g), torch.randn(T, 64, generator=g) * 1.5, torch.randn(T, 64, generator=g) * 3.0
    xr, sr = P.res_skip_ref(o, x, sk, dtype=torch.float32)
    x64, s64 = P.res_skip_ref(o, x, sk)
    assert (xr.double() - x64).abs().max() <= 2.0 ** -23 * x64.abs().max() and (sr.double() - s64).abs().max() <= 2.0 ** -24 * s64.abs().max()
    gx, gs, od = Guarded(x), Guarded(sk), o.to(DEV)
    ops.pwg_res_skip(od, gx.t, gs.t)
    torch.cuda.synchronize()
    assert gx.intact() and gs.intact() and _same_bits(od.cpu(), o)
    assert _same_bits(gx.t.cpu(), xr) and _same_bits(gs.t.cpu(), sr)


@pytest.mark.parametrize("shape", [(3, 7, 5, 3, (3, 0, 1), 2), (3, 1100, 80, 4, (550, 150, 0), 2)], ids=["small", "past_one_trip"])
def test_pwg_upsample_dense_and_ragged(shape):
    """Dense and ragged against the fp32 restatement in the kernel's order of additions (bit for bit) and against float64; a
    ragged row against the dense launch of the row alone; zeros behind a row."""
    from a3t_amd import ops
    B, Tin, C, scale, lens, mul = shape
    g = torch.Generator().manual_seed(13)
    c, w = torch.randn(B, Tin, C, generator=g), torch.rand(2 * scale + 1, generator=g)
    w = w / w.sum()
    wd = w.to(DEV)
    out = Guarded(shape=(B, Tin * scale, C), fill=float("nan"))
    ops.pwg_upsample(c.to(DEV), wd, out.t, scale)
    torch.cuda.synchronize()
    assert out.intact() and _same_bits(out.t.cpu(), P.upsample_ref(c, w, scale, dtype=torch.float32))
    bound = (2 * scale + 2) * 2.0 ** -24 * float(c.abs().max())
    assert (out.t.cpu().double() - P.upsample_ref(c, w, scale)).abs().max() <= bound
    cn = c.clone()
    for b, n in enumerate(lens):
        cn[b, n * mul:] = float("nan")
    rag = Guarded(shape=(B, Tin * scale, C), fill=float("nan"))
    ops.pwg_upsample(cn.to(DEV), wd, rag.t, scale, torch.tensor(lens, dtype=torch.int32, device=DEV), mul)
    torch.cuda.synchronize()
    got = rag.t.cpu()
    assert rag.intact() and _same_bits(got, P.upsample_ref(cn, w, scale, lens, mul, dtype=torch.float32))
    for b, n in enumerate(lens):
        L = n * mul
        assert bool((got[b, L * scale:] == 0).all())
        if L:
            alone = torch.empty(L * scale, C, device=DEV)
            ops.pwg_upsample(c[b, :L].contiguous().to(DEV), wd, alone, scale)
            assert _same_bits(got[b, :L * scale], alone.cpu())


@pytest.mark.parametrize("shape", [(3, 12, 5, 4, (12, 6, 0)), (3, 4400, 80, 2, (4400, 1, 1700))], ids=["small", "past_one_trip"])
def test_replicate_pad_dense_and_ragged(shape):
    from a3t_amd import ops
    B, T, C, pad, lens = shape
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(14))
    y = Guarded(shape=(B, T + 2 * pad, C), fill=float("nan"))
    ops.replicate_pad(x.to(DEV), y.t, pad)
    torch.cuda.synchronize()
    assert y.intact() and _same_bits(y.t.cpu(), P.replicate_pad_ref(x, pad))
    xn = x.clone()
    for b, n in enumerate(lens):
        xn[b, n:] = float("nan")
    y = Guarded(shape=(B, T + 2 * pad, C), fill=float("nan"))
    ops.replicate_pad(xn.to(DEV), y.t, pad, torch.tensor(lens, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    got = y.t.cpu()
    assert y.intact() and _same_bits(got, P.replicate_pad_ref(xn, pad, lens)) and bool(torch.isfinite(got).all())
    for b, n in enumerate(lens):
        if n:
            alone = torch.empty(n + 2 * pad, C, device=DEV)
            ops.replicate_pad(x[b, :n].contiguous().to(DEV), alone, pad)
            assert _same_bits(got[b, :n + 2 * pad], alone.cpu())


def test_zero_tail():
    """NaN tails become zero, heads keep their bits; rows of length 0 and T; past one grid-stride trip."""
    from a3t_amd import ops
    B, T, C, mul = 4, 4500, 64, 3
    lens = (0, 1500, 700, 1)
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(15))
    for b, n in enumerate(lens):
        x[b, n * mul:] = float("nan")
    x[1, 0, 0] = -0.0
    gx = Guarded(x)
    ops.zero_tail(gx.t, torch.tensor(lens, dtype=torch.int32, device=DEV), mul, B, T)
    torch.cuda.synchronize()
    got = gx.t.cpu()
    assert gx.intact() and _same_bits(got, P.zero_tail_ref(x, lens, mul))
    assert bool((got[0] == 0).all()) and _same_bits(got[1], x[1]) and not torch.isnan(got).any()


def test_reflect_pad_rows_ragged():
    """Bit-exact against torch's reflection of the row alone: a full row, the shortest length one reflection reaches (pad + 1), an
    empty row; at a rate of 3 samples per frame as well."""
    from a3t_amd import ops
    C, T, pad = 5, 12, 4
    x = torch.randn(4, T, C, generator=torch.Generator().manual_seed(16))
    for lens, mul in (((12, 5, 0, 7), 1), ((4, 2, 0, 3), 3)):
        xn = x.clone()
        for b, n in enumerate(lens):
            xn[b, n * mul:] = float("nan")
        y = Guarded(shape=(4, T + 2 * pad, C), fill=float("nan"))
        ops.reflect_pad_rows(xn.to(DEV), y.t, pad, torch.tensor(lens, dtype=torch.int32, device=DEV), mul)
        torch.cuda.synchronize()
        got = y.t.cpu()
        assert y.intact() and _same_bits(got, P.reflect_pad_rows_ref(xn, pad, lens, mul)) and bool(torch.isfinite(got).all())
        for b, n in enumerate(lens):
            L = n * mul
            if L:
                want = F.pad(x[b, :L].t()[None], (pad, pad), mode="reflect")[0].t()
                assert _same_bits(got[b, :L + 2 * pad], want)
            else:
                assert bool((got[b] == 0).all())


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def test_block_entry_points_refuse_without_launching():
    """dil = 0, a null operand, B = 0, a misaligned tile list, a list with ntiles < 0, no list for the ragged entry point, and an
    operand that is read as float4 but is not 16-byte aligned: A3T_EINVAL, and x, g, skips keep every bit."""
    from a3t_amd import _lib, ops
    from a3t_amd.ops import _ptr, _stream
    lib = _lib.load()
    _, dev, _ = _operands()
    B, Tw = 1, 300
    n = B * Tw
    pad = 4                                                    # spare floats for the offset views
    bufs = {k: torch.full((n * C + pad,), 5.0, device=DEV) for k, C in (("x", 64), ("cu", 80), ("g", 64), ("sk", 64))}
    w = {k: torch.cat([t.reshape(-1), t.new_zeros(pad)]) for k, t in zip(("wt0", "b0", "wt1", "b1"), dev)}
    tl = torch.zeros(8, dtype=torch.int32, device=DEV)
    tl[:4] = torch.tensor([0, 0, Tw, 0], dtype=torch.int32)
    tl[4:] = torch.tensor([0, 256, Tw, 0], dtype=torch.int32)
    mis = torch.zeros(9, dtype=torch.int32, device=DEV)
    mis[1:] = tl

    def args(off=None, null=None):
        names = ("x", "cu", "wt0", "b0", "wt1", "b1", "g", "sk")
        ts = [(bufs | w)[k][(1 if k == off else 0):] for k in names]
        return [None if k == null else _ptr(t) for k, t in zip(names, ts)]

    def dense(a, B=B, Tw=Tw, dil=1):
        return lib.a3t_pwg_block(*a, B, Tw, dil, _stream())

    def ragged(a, tiles, ntiles, B=B, Tw=Tw, dil=1):
        return lib.a3t_pwg_block_ragged(*a, tiles, ntiles, B, Tw, dil, _stream())

    assert dense(args(), dil=0) == EINVAL and dense(args(), dil=-1) == EINVAL
    assert dense(args(), B=0) == EINVAL and dense(args(), Tw=0) == EINVAL
    assert ragged(args(), _ptr(tl), 2, dil=0) == EINVAL and ragged(args(), _ptr(tl), 2, B=0) == EINVAL
    for k in ("x", "cu", "wt0", "b0", "wt1", "b1", "g", "sk"):
        assert dense(args(null=k)) == EINVAL and ragged(args(null=k), _ptr(tl), 2) == EINVAL, k
    assert ragged(args(), _ptr(mis[1:]), 2) == EINVAL
    assert ragged(args(), _ptr(tl), -1) == EINVAL
    assert ragged(args(), None, 0) == EINVAL and ragged(args(), None, 2) == EINVAL
    for k in ("x", "cu", "g", "wt0", "wt1"):                   # read as float4
        assert dense(args(off=k)) == EINVAL and ragged(args(off=k), _ptr(tl), 2) == EINVAL, k
    torch.cuda.synchronize()
    assert all(bool((t == 5.0).all()) for t in bufs.values())
    # the same through ops, with an offset view that passes every check of the wrapper
    view = {k: (t[:n * C].view(n, C), t[1:n * C + 1].view(n, C)) for (k, t), C in zip(bufs.items(), (64, 80, 64, 64))}
    for k in ("x", "cu", "g"):
        a = {j: view[j][1 if j == k else 0] for j in view}
        with pytest.raises(_lib.A3TLibraryError):
            ops.pwg_block(a["x"], a["cu"], *dev, a["g"], a["sk"], B, Tw, 1)
    torch.cuda.synchronize()
    assert all(bool((t == 5.0).all()) for t in bufs.values())
    ops.pwg_block(view["x"][0], view["cu"][0], *dev, view["g"][0], view["sk"][0], B, Tw, 1, tl.view(2, 4))   # the good call goes through
    torch.cuda.synchronize()
    assert bool(torch.isfinite(bufs["x"]).all()) and not bool((bufs["x"][:n * 64] == 5.0).all())
