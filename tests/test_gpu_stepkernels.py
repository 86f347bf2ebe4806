"""The step kernels of csrc/misc.hip (loss, gradient norm, clip+Adam, dropout, encoder prologue, casts and element-wise helpers)
against tests/stepkernel_ref.py, one test per case of its table, plus the dropout masks of every other user of the generator
against the numpy restatement.

Every output lives between two guard bands of a sentinel, which must come back untouched; every input must come back bit for bit.
Copies, casts and one- or two-rounding arithmetic are compared bit for bit (NaN by isnan), accumulating kernels against
|got - ref| <= (L 2^-23 + 2 r) mag with L counted in stepkernel_ref.  Each test prints `max error / bound` per output (pytest -s
shows it); a ratio above 1 fails.  Each case runs twice: outputs that involve no atomic must be bit-equal.
Run with `pytest -m gpu` on an MI355X."""
import math

import numpy as np
import pytest
import torch

import gemm_ref as G
import rowkernel_ref as RK
import stepkernel_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256                # elements in front of and behind every output
SENT = -1536.0             # exact in bf16, fp32, fp64 and the signed integers
SENT_U8 = 0xA5
F32 = np.float32
ATOMIC = {"colsum", "demb", "dseg", "gbqkv"}


def _ops():
    from a3t_amd import ops
    return ops


def _lib():
    from a3t_amd import _lib
    return _lib.load()


def _sent(dtype):
    return SENT_U8 if dtype == torch.uint8 else SENT


def _tt(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


class Bands:
    """Allocates the outputs of one case and checks their guard bands afterwards."""

    def __init__(self):
        self.made = []

    def out(self, shape, dtype=torch.float32, init=None, offset=0):
        n = int(np.prod(shape)) if len(shape) else 1
        buf = torch.full((GUARD + offset + n + GUARD,), _sent(dtype), dtype=dtype, device=DEV)
        view = buf[GUARD + offset:GUARD + offset + n].view(*shape)
        if init is not None:
            view.copy_(_tt(init).reshape(shape)) if not np.isscalar(init) else view.fill_(init)
        self.made.append((buf, GUARD + offset, n))
        return view

    def intact(self):
        torch.cuda.synchronize()
        for buf, lo, n in self.made:
            s = _sent(buf.dtype)
            assert bool((buf[:lo] == s).all()) and bool((buf[lo + n:] == s).all()), "a guard band was written"


class Inputs:
    """Device copies of the operands; `unchanged` compares them bit for bit with what went in."""

    def __init__(self):
        self.made = []

    def __call__(self, a, offset=0):
        if a is None:
            return None
        t = _tt(a)
        buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
        view = buf[offset:].view(t.shape)
        view.copy_(t)
        self.made.append((view, t))
        return view

    def unchanged(self, cid):
        for view, t in self.made:
            _bits(cid, "an input", view, t)


def _bits(cid, name, got, exp):
    g, e = got.detach().cpu().reshape(-1), _tt(exp).reshape(-1)
    assert g.dtype == e.dtype and g.numel() == e.numel(), (cid, name, g.dtype, e.dtype, g.numel(), e.numel())
    if g.dtype.is_floating_point:
        gn, en = torch.isnan(g), torch.isnan(e)
        iv = {4: torch.int32, 2: torch.int16, 8: torch.int64}[g.element_size()]
        bad = (gn != en) | ((g.view(iv) != e.view(iv)) & ~gn)
    else:
        bad = g != e
    if bool(bad.any()):
        at = bad.nonzero().flatten()[:8]
        raise AssertionError(f"{cid} {name}: {int(bad.sum())} of {g.numel()} differ, first at {at.tolist()}: got {g[at].tolist()} expected {e[at].tolist()}")


def _ratio(case, name, got, o):
    g = got.detach().cpu().to(torch.float64).numpy().reshape(np.shape(o.ref))
    assert np.isfinite(g).all(), (case["id"], name, "not finite")
    b = S.bound(o)
    ratio = float(np.max(np.abs(g - o.ref) / np.maximum(b, 1e-300))) if g.size else 0.0
    print(f"RATIO {case['op']} [{case['id']}] {name}: max error / bound = {ratio:.3f}  (L = {o.L}, r = {o.r:.2e})")
    assert ratio <= 1.0, (case["id"], case["label"], name, ratio)


def _check(case, name, got, exp):
    if isinstance(exp, S.Approx):
        _ratio(case, name, got, exp)
    else:
        _bits(case["id"], name, got, exp)


def _rc(rc):
    assert rc == S.EINVAL, rc
    torch.cuda.synchronize()


TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


# ---- one runner per op: returns name -> (device tensor, expected) ------------------------------------------------------
def run_loss(c, i, dev, bands):
    ops, M, C = _ops(), c["M"], c["C"]
    before, after, target, masked = dev(i["before"]), dev(i["after"]), dev(i["target"]), dev(i["masked"])
    loss = bands.out((1,))
    scratch = bands.out((ops.loss_scratch_floats(M),))
    db = bands.out((M, C)) if c["want"][0] else None
    da = bands.out((M, C)) if c["want"][1] else None
    ops.mlm_loss(before, after, target, masked, loss, db, da, scratch, l2=bool(c["l2"]), gscale=c["gscale"])
    r = S.mlm_loss_ref(i["before"], i["after"], i["target"], i["masked"], c["l2"], c["gscale"], c["want"])
    res = dict(loss=(loss, S.Approx(np.array([r["loss"]]), np.array([r["mag"]]), S.loss_L(M, C), 0.0)))
    for name, buf, g in (("d_before", db, r["d_before"]), ("d_after", da, r["d_after"])):
        if buf is not None:      # a buffer that is given but not to be written keeps its sentinel
            res[name] = (buf, g if g is not None else np.full((M, C), SENT, F32))
    return res


def run_sumsq(c, i, dev, bands):
    n = c["n"]
    if c.get("device_made"):
        g = torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(S.seed_of(c["id"])))
        ref = float(g.double().pow(2).sum().sqrt())
    else:
        g = dev(i["g"], 0 if c["aligned"] else 1)
        ref = math.sqrt(S.sumsq_ref(i["g"]))
    assert (g.data_ptr() % 16 == 0) == c["aligned"]
    partial = bands.out((S.SUMSQ_BLOCKS,), torch.float64)
    _ops().sumsq(g, partial)
    return dict(norm=(partial.sum().sqrt().float().reshape(1), S.Approx(np.array([ref]), np.array([ref]), S.norm_L(n, c["aligned"]), 0.0)))


def run_adam(c, i, dev, bands):
    ops, n, t = _ops(), c["n"], c["t"]
    oa = 1 if c["offset"] == "all" else 0
    g = dev(i["g"], 1 if c["offset"] != "none" else 0)
    partial = bands.out((S.SUMSQ_BLOCKS,), torch.float64)
    ops.sumsq(g, partial)
    res = {}
    for name, lr in S.adam_entries():
        p, m, v = (bands.out((n,), init=i[k], offset=oa) for k in "pmv")
        assert all((x.data_ptr() % 16 == 0) == (oa == 0) for x in (p, m, v)) and (g.data_ptr() % 16 == 0) == c["aligned"]
        norm = bands.out((1,))
        o = S.adam_ref(i["p"], i["g"], i["m"], i["v"], t, lr, c["clip"], c["gscale"], aligned=c["aligned"])
        if name == "host":
            ops.clip_adam(p, g, m, v, partial, norm, lr, t, clip=c["clip"], gscale=c["gscale"])
        else:
            state = bands.out((2,), torch.int32, init=np.array([t - 1, 0], np.int32))
            ops.clip_adam_noam(p, g, m, v, partial, norm, state, lr[0], lr[1], lr[2], clip=c["clip"], gscale=c["gscale"])
            res[f"{name}.clock"] = (state, np.array([t - 1, 1] if o["skip"] else [t, 0], np.int32))
        if o["skip"]:
            torch.cuda.synchronize()
            assert not math.isfinite(float(norm)), (c["id"], name)
            for k, x in zip("pmv", (p, m, v)):
                res[f"{name}.{k}"] = (x, i[k])
        else:
            res[f"{name}.norm"] = (norm, S.Approx(np.array([o["norm"].ref]), np.array([o["norm"].mag]), o["norm"].L, 0.0))
            for k, x in zip("pmv", (p, m, v)):
                res[f"{name}.{k}"] = (x, o[k])
    return res


def run_dropout(c, i, dev, bands):
    ops, n, p, key = _ops(), c["n"], c["p"], c["key"]
    x = dev(i["x"])
    y = bands.out((n,), TDT[c["io"][1]])
    ops.dropout(x, y, p, key, c["scale"])
    res = dict(y=(y, S.dropout_exact(i["x"], p, key, c["scale"], c["io"][1])))
    if c["io"] == ("f32", "f32"):      # the mask itself, read off a tensor of ones
        ones = bands.out((n,), init=1.0)
        y1 = bands.out((n,))
        ops.dropout(ones, y1, p, key)
        res["mask"] = (y1 != 0, S.keep_mask(key, n, p))
    return res


def run_dropout_bwd_cast(c, i, dev, bands):
    M, C = c["M"], c["C"]
    g = dev(i["g"])
    gm = bands.out((M, C), TDT[c["kind"]])
    colsum = bands.out((C,), init=i["colsum0"]) if i["colsum0"] is not None else None
    _ops().dropout_bwd_cast(g, gm, c["p"], c["key"], colsum, c["colsum_scale"])
    r = S.dropout_bwd_cast_ref(i["g"], c["p"], c["key"], i["colsum0"], c["colsum_scale"], c["kind"])
    res = dict(gm=(gm, r["gm"]))
    if colsum is not None:
        res["colsum"] = (colsum, r["colsum"])
    return res


def run_embed_fwd(c, i, dev, bands):
    B, Tm, Tp, D = (c[k] for k in ("B", "Tm", "Tp", "D"))
    seg, spk = (i["seg"] if c["seg"] else None), (i["spk"] if c["spk"] else None)
    xs = bands.out((B * (Tm + Tp), D))
    _ops().embed_finish_fwd(dev(i["e"]), dev(i["emb"]), dev(seg), dev(i["text"]), dev(i["spos"]), dev(i["tpos"]), xs, B, Tm, Tp, D, i["xscale"],
                            drop=(c["p"], c["key"]), spk=dev(spk))
    return dict(xs=(xs, S.embed_finish_fwd_exact(i["e"], i["emb"], seg, i["text"], i["spos"], i["tpos"], B, Tm, Tp, D, i["xscale"], c["p"], c["key"],
                                                 spk)))


def run_embed_bwd(c, i, dev, bands):
    B, Tm, Tp, D, V, nseg = tuple(c[k] for k in ("B", "Tm", "Tp", "D")) + (i["V"], i["nseg"])
    de = bands.out((B * Tm, D))
    demb = bands.out((V, D), init=i["demb0"])
    dseg = bands.out((nseg, D), init=i["dseg0"]) if c["seg"] else None
    _ops().embed_finish_bwd(dev(i["dxs"]), dev(i["e"]), dev(i["text"]), dev(i["spos"]), dev(i["tpos"]), de, demb, dseg, B, Tm, Tp, D, V, nseg,
                            i["xscale"], drop=(c["p"], c["key"]))
    r = S.embed_finish_bwd_ref(i["dxs"], i["e"], i["text"], i["spos"], i["tpos"], B, Tm, Tp, D, V, nseg, i["xscale"], c["p"], c["key"], c["seg"],
                               i["demb0"], i["dseg0"])
    res = dict(de=(de, r["de"]), demb=(demb, r["demb"]))
    if dseg is not None:
        res["dseg"] = (dseg, r["dseg"])
    return res


def run_cast_conv_t(c, i, dev, bands):
    N, taps, C = c["N"], c["taps"], c["C"]
    src = dev(i["src"])
    assert src.data_ptr() % 16 == 0 and all(int(o) % 4 for o in i["src_off"])
    dst = bands.out((i["dst_len"],), torch.bfloat16)
    _ops().cast_bf16_conv_t(src, dst, dev(i["src_off"]), dev(i["dst_off"]), N, taps, C)
    exp = torch.full((i["dst_len"],), SENT, dtype=torch.bfloat16)       # sentinels in front of, between and behind the shadows
    for so, do in zip(i["src_off"], i["dst_off"]):
        exp[do:do + N * taps * C] = S.cast_conv_t_exact(i["src"][so:so + N * taps * C].reshape(N, taps, C)).reshape(-1)
    return dict(dst=(dst, exp))


def run_cast_bf16(c, i, dev, bands):
    y = bands.out((c["n"],), torch.bfloat16)
    _ops().cast_bf16(dev(i["x"]), y)
    return dict(y=(y, S.bf16(i["x"])))


def run_split_bf16(c, i, dev, bands):
    hi, lo = bands.out((c["n"],), torch.bfloat16), bands.out((c["n"],), torch.bfloat16)
    _ops().split_bf16(dev(i["x"]), hi, lo)
    eh, el = S.split_bf16_exact(i["x"])
    return dict(hi=(hi, eh), lo=(lo, el))


def run_slice_rows(c, i, dev, bands):
    B, T, Tm, D = (c[k] for k in ("B", "T", "Tm", "D"))
    if c["reverse"]:
        x = bands.out((B * T, D), init=i["x"])
        _ops().slice_rows(x, dev(i["y"]), B, T, Tm, D, reverse_add=True)
        return dict(x=(x, S.slice_rows_reverse_exact(i["x"], i["y"], B, T, Tm, D)))
    y = bands.out((B * Tm, D), TDT[c["kind"]])
    _ops().slice_rows(dev(i["x"]), y, B, T, Tm, D)
    return dict(y=(y, S.slice_rows_exact(i["x"], B, T, Tm, D, c["kind"])))


def run_scale(c, i, dev, bands):
    ops, n = _ops(), c["n"]
    x = bands.out((n,), init=i["x"]) if c["inplace"] else dev(i["x"])
    y = x if c["inplace"] else bands.out((n,))
    if c["op"] == "scale":
        ops.scale(x, y, i["s"])
    else:
        ops.scale_dev(x, y, dev(np.array([i["s"]], F32)))
    return dict(y=(y, S.scale_exact(i["x"], i["s"])))


def run_axpy(c, i, dev, bands):
    y = bands.out((c["n"],), init=i["y"])
    _ops().axpy(dev(i["x"]), y, i["s"])
    return dict(y=(y, S.axpy_exact(i["x"], i["y"], i["s"])))


def run_mask_fill(c, i, dev, bands):
    out = bands.out((c["M"], c["C"]), TDT[c["kind"]])
    _ops().mask_fill(dev(i["x"]), dev(i["masked"]), dev(i["mf"]), out)
    return dict(out=(out, S.mask_fill_exact(i["x"], i["masked"], i["mf"], c["kind"])))


def run_bias_act(c, i, dev, bands):
    x = bands.out((c["M"], c["C"]), init=i["x"])
    _ops().bias_act(x, dev(i["bias"]), c["act"], c["scale"])
    return dict(x=(x, S.bias_act_ref(i["x"], i["bias"], c["act"], c["scale"])))


def run_segment_colsum(c, i, dev, bands):
    out = bands.out((c["B"], c["C"]), init=i["out0"])
    _ops().segment_colsum(dev(i["x"]), out, c["B"], c["T"])
    return dict(out=(out, S.segment_colsum_ref(i["x"], i["out0"], c["B"], c["T"])))


def run_attn_bias_fold(c, i, dev, bands):
    d = c["d"]
    gu, gv, gb = bands.out((d,), init=i["gu0"]), bands.out((d,), init=i["gv0"]), bands.out((3 * d,), init=i["gb0"])
    _ops().attn_bias_fold(dev(i["slots"]), c["S"], d, gu, gv, gb)
    r = S.attn_bias_fold_ref(i["slots"], c["S"], d, i["gu0"], i["gv0"], i["gb0"])
    return dict(gu=(gu, r["gu"]), gv=(gv, r["gv"]), gbqkv=(gb, r["gbqkv"]))


def run_splice_spans(c, i, dev, bands):
    B, Tout, C = c["B"], c["Tout"], c["C"]
    out, lens = bands.out((B, Tout, C)), bands.out((B,), torch.int32)
    _ops().splice_spans(dev(i["after"]), dev(i["speech"]), dev(i["mask"]), dev(i["spans"]), out, lens)
    eo, el = S.splice_spans_exact(i["after"], i["speech"], i["mask"], i["spans"], Tout)
    return dict(out=(out, eo), lens=(lens, el))


def run_collate_paint(c, i, dev, bands):
    B, Tm, Tp = c["B"], c["Tm"], c["Tp"]
    masked, smask, tmask = bands.out((B, Tm), torch.uint8), bands.out((B, Tm), torch.uint8), bands.out((B, Tp), torch.uint8)
    sp, tp = bands.out((B, Tm), torch.int64), bands.out((B, Tp), torch.int64)
    _ops().collate_paint(dev(i["fs"]), dev(i["fe"]), dev(i["alen"]), dev(i["sel"]), dev(i["mspan"]), dev(i["nms"]), dev(i["flen"]), dev(i["tlen"]),
                         masked, smask, tmask, sp, tp, c["sega"])
    e = S.collate_paint_exact(i["fs"], i["fe"], i["alen"], i["sel"], i["mspan"], i["nms"], i["flen"], i["tlen"], Tm, Tp, c["sega"])
    return dict(masked=(masked, e["masked"]), smask=(smask, e["smask"]), tmask=(tmask, e["tmask"]), sp=(sp, e["sp"]), tp=(tp, e["tp"]))


RUN = {"loss": run_loss, "sumsq": run_sumsq, "adam": run_adam, "dropout": run_dropout, "dropout_bwd_cast": run_dropout_bwd_cast,
       "embed_fwd": run_embed_fwd, "embed_bwd": run_embed_bwd, "cast_conv_t": run_cast_conv_t, "cast_bf16": run_cast_bf16,
       "split_bf16": run_split_bf16, "slice_rows": run_slice_rows, "scale": run_scale, "scale_dev": run_scale, "axpy": run_axpy,
       "mask_fill": run_mask_fill, "bias_act": run_bias_act, "segment_colsum": run_segment_colsum, "attn_bias_fold": run_attn_bias_fold,
       "splice_spans": run_splice_spans, "collate_paint": run_collate_paint}


@pytest.mark.parametrize("cid", [c["id"] for c in S.CASES])
def test_stepkernel_case(cid):
    case = S.CASE_BY_ID[cid]
    assert S.predicted_label(case) == case["label"]
    inp = S.make_inputs(case)
    first = None
    for rep in range(2):
        bands, dev = Bands(), Inputs()
        res = RUN[case["op"]](case, inp, dev, bands)
        bands.intact()
        dev.unchanged(cid)
        if rep == 0:
            for name, (got, exp) in res.items():
                _check(case, name, got, exp)
            first = res
        else:      # the second run: bit-equal wherever no atomic is involved
            for name, (got, _) in res.items():
                if name.split(".")[-1] not in ATOMIC:
                    _bits(cid, f"{name} (second run)", got, first[name][0].detach().cpu())


# ---- refusals: arguments an entry point checks before it launches ------------------------------------------------------
def test_refusals():
    ops, lib = _ops(), _lib()
    P, st = ops._ptr, ops._stream()
    x = torch.zeros(64, device=DEV)
    u8 = torch.ones(8, dtype=torch.uint8, device=DEV)
    sc = torch.zeros(ops.loss_scratch_floats(4), device=DEV)
    good = [P(x), P(x), P(x), P(u8), P(x), None, None, P(sc)]
    for M, C in ((0, 8), (8, 0), (-1, 8)):
        _rc(lib.a3t_mlm_loss(*good, M, C, 0, 1.0, st))
    for missing in (0, 2, 3, 4, 7):      # before, target, masked, loss_out, scratch
        a = list(good)
        a[missing] = None
        _rc(lib.a3t_mlm_loss(*a, 4, 8, 0, 1.0, st))
    for M, C in ((0, 8), (8, 0), (65536 * S.RPB, 1)):      # nothing to do; more row blocks than grid.y holds
        _rc(lib.a3t_dropout_bwd_cast(P(x), P(x), 0, None, 1.0, M, C, 0.1, 1, st))
    _rc(lib.a3t_dropout_bwd_cast(P(x), P(x), 0, None, 1.0, 4, 8, 1.0, 1, st))
    _rc(lib.a3t_dropout(P(x), 0, P(x), 0, 8, 1.0, 1, 1.0, st))
    off = torch.zeros(4, dtype=torch.int64, device=DEV)
    for count, N, taps, C in ((1, 1, 65536, 1), (65536, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        _rc(lib.a3t_cast_bf16_conv_t(P(x), P(x), P(off), P(off), count, N, taps, C, st))
    _rc(lib.a3t_cast_bf16(P(x), P(x), 6, st))
    _rc(lib.a3t_split_bf16(P(x), P(x), P(x), 6, st))
    _rc(lib.a3t_cast_bf16(P(x[1:]), P(x), 8, st))
    _rc(lib.a3t_segment_colsum(P(x), P(x), 65536, 1, 1, st))
    _rc(lib.a3t_segment_colsum(P(x), P(x), 1, 0, 1, st))
    _rc(lib.a3t_attn_bias_fold(P(x), 0, 4, P(x), P(x), P(x), st))
    _rc(lib.a3t_splice_spans(P(x), P(x), P(u8), P(x), P(x), P(x), 0, 4, 4, 1, st))
    _rc(lib.a3t_collate_paint(*([P(x)] * 13), 1, 0, 1, 1, 1, 1, st))
    assert bool((x == 0).all()) and bool((sc == 0).all()) and bool((u8 == 1).all())


# ---- the other users of the generator: zero pattern == numpy mask at the kernel's index rule ---------------------------------
def _mask_eq(what, zero_pattern_kept, key, n, p, where=None):
    got = zero_pattern_kept.detach().cpu().reshape(-1).numpy()
    exp = S.keep_mask(key, n, p)
    ok = np.ones(n, bool) if where is None else where.detach().cpu().reshape(-1).numpy()
    bad = (got != exp) & ok
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:8].tolist())
    print(f"MASK {what}: {int(ok.sum())} elements, kept {int((got & ok).sum())}, equal to the numpy mask")


@pytest.mark.parametrize("M,N,K", [(5, 7, 64), (300, 256, 64)])
def test_gemm_epilogue_mask_scalar_and_vector(M, N, K):
    """linear_fwd(drop=(p, key)): the epilogue indexes the generator with the linear index m * N + n of C."""
    ops, p, key = _ops(), 0.3, 0x1234abcd
    gen = torch.Generator().manual_seed(M)
    x, W = torch.ones(M, K, device=DEV), (torch.rand(N, K, generator=gen) + 0.5).to(DEV)
    bands = Bands()
    out = bands.out((M, N))
    ops.linear_fwd(x, W, out, drop=(p, key))
    bands.intact()
    _mask_eq(f"linear_fwd {M}x{N}x{K} {_lib().a3t_gemm_last_kernel().decode()}", out != 0, key, M * N, p)
    ref = (W.double().sum(1)[None, :].expand(M, N) * float(S.drop_inv(p))).cpu()
    kept = torch.from_numpy(S.keep_mask(key, M * N, p)).view(M, N)
    assert bool(((out.cpu().double() - ref).abs()[kept] <= (K + 8) * S.U23 * ref[kept]).all())


@pytest.mark.parametrize("route", ["f32", "glds", "8p", "pn"])
def test_gemm_route_dropout_cases_with_the_numpy_mask(route):
    """The dropout cases of the exact GEMM tables (the smallest shapes those routes are tested at), with the keep mask taken from
    the numpy generator instead of from ops.dropout: C must still be exact, sentinels included."""
    ops, lib = _ops(), _lib()
    if route == "f32":
        mode, cases, prefix = "default", G.f32_epilogue_cases(), "gemm_f32_kernel"
    else:
        mode, cases, prefix = G.bf16_route_table()[{"glds": 0, "8p": 1, "pn": 4}[route]]
    cases = [c for c in cases if c.kw.get("drop") and c.kw["drop"][0] > 0]
    assert cases, route
    old = G.set_modes(lib, G.MODES[mode])
    try:
        for case in cases:
            t, base = case.place(DEV)
            case.call(ops.gemm, t)
            torch.cuda.synchronize()
            assert lib.a3t_gemm_last_kernel().decode().startswith(prefix + "<"), (route, case.name)
            host, _ = case.place("cpu")
            p, key = case.kw["drop"]
            keep = torch.from_numpy(S.keep_mask(key, host["C"].numel(), p).astype(np.float32))
            ref = case.reference(host, keep=keep)
            buf, off = case.bufs["C"]
            exp = buf.clone()
            exp[off:] = ref.C.to(buf.dtype)
            assert torch.equal(base["C"].cpu(), exp), (route, case.name)
            print(f"MASK gemm {route} '{case.name}' {lib.a3t_gemm_last_kernel().decode()}: C exact with the numpy mask")
    finally:
        G.set_modes(lib, old)


@pytest.mark.parametrize("T,dt,path", [(70, "f32", "relpos_softmax_fwd<NV=2>"), (2049, "f32", "relpos_softmax_fwd<NV=0>"),
                                       (72, "bf16", "relpos_softmax_fwd_bf16<NC=1>")])
def test_relpos_softmax_probs_drop_mask(T, dt, path):
    """probs_drop on the register path (NV > 0), the looping path (T > 2048) and the bf16 kernel: the linear index of probs."""
    B, H, p, key = (1, 1, 0.1, 0x9e3779b9) if T > 2048 else (2, 2, 0.1, 0x9e3779b9)
    zero = torch.zeros(B, H, T, T, dtype=TDT[dt], device=DEV)
    bands = Bands()
    probs, pdrop = bands.out((B, H, T, T), TDT[dt]), bands.out((B, H, T, T), TDT[dt])
    _ops().relpos_softmax_fwd(zero, zero, torch.ones(B, T, dtype=torch.uint8, device=DEV), probs, B, H, T, 1.0, probs_drop=pdrop, drop=(p, key))
    bands.intact()
    assert bool((probs != 0).all())
    label = RK.expected_path("relpos_softmax_fwd", dict(B=B, H=H, T=T), dict(s=dt, p=dt))[0]
    assert label.startswith(path), label
    _mask_eq(f"{label} T={T}", pdrop != 0, key, B * H * T * T, p)


def test_layernorm_bwd_consumer_mask():
    """The fused consumer of the LayerNorm backward: dx16 carries keep * dx / (1 - p) at the linear index row * D + c."""
    ops = _ops()
    case = next(c for c in RK.CASES if c["op"] == "ln_bwd" and c["options"].get("drop_p", 0.0) > 0 and not c["facts"]["rc"] and c["aligned"])
    inp, s, o = RK.make_inputs(case), case["shape"], case["options"]
    M, D = s["M"], s["D"]
    dy, x, g, mean, rstd, dres = (None if inp[k] is None else inp[k].to(DEV).contiguous() for k in ("dy", "x", "g", "mean", "rstd", "dres"))
    bands = Bands()
    dx, dx16 = bands.out((M, D)), bands.out((M, D), torch.bfloat16)
    dg, db = bands.out((D,), init=0.0), bands.out((D,), init=0.0)
    ops.layernorm_bwd(dy, x, g, mean, rstd, dres, dx, dg, db, dx16=dx16, drop=(o["drop_p"], o["drop_key"]))
    bands.intact()
    _mask_eq(f"ln_bwd consumer {case['label']}", dx16 != 0, o["drop_key"], M * D, o["drop_p"], where=dx.to(torch.bfloat16) != 0)


def test_fused_attention_single_tensor_save_sign_bits_are_the_numpy_mask():
    """a3t_attn_fwd_train without probs_drop stores one [B][H][T][T] tensor whose sign bits carry the dropout mask (set = dropped);
    the kernel indexes the generator with ((b H + h) T + i) T + j, the linear index of that tensor."""
    B, H, T, dk, p, key = 2, 2, 136, 32, 0.2, 0xC0FFEE
    d, M = H * dk, B * T
    rs = np.random.RandomState(3 * T + dk)
    mk = lambda *s, sc=1.0: torch.from_numpy((rs.standard_normal(s) * sc).astype(F32)).to(DEV).bfloat16()      # noqa: E731
    qkv = mk(M, 3 * d)
    qu = (qkv[:, :d].float() + mk(1, d, sc=0.3).float()).bfloat16().contiguous()
    qv = (qkv[:, :d].float() + mk(1, d, sc=0.3).float()).bfloat16().contiguous()
    P = mk(T, d)
    bands = Bands()
    ctx, lse, rsum = bands.out((M, d), torch.bfloat16), bands.out((B, H, T)), bands.out((B, H, T))
    probs = bands.out((B, H, T, T), torch.bfloat16)
    _ops().attn_fwd_train(qu, qv, qkv, P, torch.ones(B, T, dtype=torch.uint8, device=DEV), ctx, lse, probs, None, rsum, B, H, T,
                          1.0 / math.sqrt(dk), drop=(p, key))
    bands.intact()
    bits = probs.view(torch.int16)
    nz = (bits & 0x7fff) != 0
    assert float(nz.float().mean()) > 0.9
    _mask_eq("attn_fwd_train single-tensor save", bits >= 0, key, B * H * T * T, p, where=nz)
