"""Every dispatch path and loop wrap of the row kernels (LayerNorm, BatchNorm+activation, column reductions, GLU+depthwise conv,
add_pos_bias, rel-pos softmax) against the float64 references of tests/rowkernel_ref.py, one test per case of its table.

Every output lives between two guard bands of a sentinel value, which must come back untouched.  Tolerances are not set by hand:
|got - ref| <= ((L + 8) 2^-23 + 2 r) mag, see rowkernel_ref.  Each test prints `max error / bound` per output (pytest -s shows it);
a ratio above 1 fails.  Run with `pytest -m gpu` on an MI355X."""
import pytest
import torch

import rowkernel_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256                # elements in front of and behind every output
SENT = -1536.0             # exact in bf16, fp32 and fp64
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _ops():
    from a3t_amd import ops
    return ops


class Bands:
    """Allocates the outputs of one case and checks their guard bands afterwards."""

    def __init__(self):
        self.made = []

    def out(self, shape, dtype=torch.float32, init=None, offset=0):
        n = 1
        for d in shape:
            n *= d
        buf = torch.full((GUARD + offset + n + GUARD,), SENT, dtype=dtype, device=DEV)
        view = buf[GUARD + offset:GUARD + offset + n].view(*shape)
        if init is not None:
            view.copy_(init) if torch.is_tensor(init) else view.fill_(init)
        self.made.append((buf, GUARD + offset, n))
        return view

    def intact(self):
        torch.cuda.synchronize()
        for buf, lo, n in self.made:
            assert bool((buf[:lo] == SENT).all()) and bool((buf[lo + n:] == SENT).all()), "a guard band was written"


def _dev(t, offset=0):
    """An operand on the device; offset (elements) moves its base pointer off the 16-byte grid."""
    if t is None:
        return None
    if not offset:
        return t.to(DEV).contiguous()
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
    view = buf[offset:].view(t.shape)
    view.copy_(t)
    return view


def _kind(t):
    return {torch.float32: "f32", torch.bfloat16: "bf16", torch.float64: "f64"}[t.dtype]


def _compare(case, got, ref, r_intr=0.0):
    """got: name -> device tensor.  Prints and asserts max error / bound per output."""
    torch.cuda.synchronize()
    worst = {}
    for name, t in got.items():
        o = ref[name]
        L = case["L"][name] if isinstance(case["L"], dict) else case["L"]
        g = t.detach().to("cpu").to(torch.float64).reshape(o.ref.shape)
        assert bool(torch.isfinite(g).all()), (case["id"], name, "not finite")
        b = R.bound(o, L, _kind(t), r_intr)
        ratio = float(((g - o.ref).abs() / b.clamp_min(1e-300)).max()) if g.numel() else 0.0
        worst[name] = ratio
        print(f"RATIO {case['label']!r} [{case['id']}] {name}: max error / bound = {ratio:.3f}  (L = {L}, r = {r_intr:.2e})")
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (case["id"], case["label"], bad)


def _einval(fn):
    from a3t_amd._lib import A3TLibraryError
    with pytest.raises(A3TLibraryError, match=r"rc=-22\b"):
        fn()
    torch.cuda.synchronize()


def _keep_rate(case, keep, eligible):
    n, k = int(eligible.sum()), int((keep & eligible).sum())
    lo, hi = R.keep_rate_interval(n, case["options"]["drop_p"])
    print(f"KEEP {case['label']!r} [{case['id']}]: kept {k} of {n}, 5 sigma interval [{lo:.0f}, {hi:.0f}]")
    assert lo <= k <= hi, (case["id"], k, n, lo, hi)


def _same_instantiation(a, b):
    """Kernel lists equal up to the RAGGED template flag."""
    strip = lambda ks: [(n, tuple(x for x in t if not isinstance(x, bool))) for n, t in ks]      # noqa: E731
    return strip(a) == strip(b)


# ----------------------------------------------------------------------------------------------------------------------
def run_ln_fwd(case, inp, bands):
    ops, s, o = _ops(), case["shape"], case["options"]
    M, D = s["M"], s["D"]
    x = _dev(inp["x"], 0 if case["aligned"] else 1)
    g, b = _dev(inp["g"]), _dev(inp["b"])
    y = bands.out((M, D), TDT[case["dtypes"].get("y", "f32")])
    mean, rstd = bands.out((M,)), bands.out((M,))
    if not o.get("ragged"):
        ops.layernorm_fwd(x, g, b, y, mean, rstd, inp["eps"])
        return dict(y=y, mean=mean, rstd=rstd), {}
    B, T = o["B"], o["T"]
    ops.layernorm_fwd_ragged(x, g, b, y, mean, rstd, _dev(inp["lens"]), B, T, inp["eps"])
    # bit for bit the dense kernel on each row alone (same instantiation: D decides it)
    dense = R.expected_path("ln_fwd", dict(M=1, D=D), case["dtypes"], case["aligned"])[1]["kernels"]
    assert _same_instantiation(dense, case["facts"]["kernels"])
    for bb, n in enumerate(o["lens"]):
        if n:
            y1, m1, r1 = bands.out((n, D)), bands.out((n,)), bands.out((n,))
            ops.layernorm_fwd(x[bb * T:bb * T + n], g, b, y1, m1, r1, inp["eps"])
            assert torch.equal(y1, y[bb * T:bb * T + n]) and torch.equal(m1, mean[bb * T:bb * T + n]) \
                and torch.equal(r1, rstd[bb * T:bb * T + n]), (case["id"], bb, n)
    return dict(y=y, mean=mean, rstd=rstd), {}


def run_ln_bwd(case, inp, bands):
    ops, s, o = _ops(), case["shape"], case["options"]
    M, D = s["M"], s["D"]
    off = 0 if case["aligned"] else 1
    dy, x, g, mean, rstd, dres = _dev(inp["dy"]), _dev(inp["x"], off), _dev(inp["g"]), _dev(inp["mean"]), _dev(inp["rstd"]), _dev(inp["dres"])
    dx = bands.out((M, D))
    dx16 = bands.out((M, D), torch.bfloat16) if o.get("dx16") else None
    dg, db = bands.out((D,), init=0.0), bands.out((D,), init=0.0)
    dxsum = bands.out((D,), init=0.0) if o.get("dxsum") else None
    call = lambda: ops.layernorm_bwd(dy, x, g, mean, rstd, dres, dx, dg, db, dx16=dx16, dxsum=dxsum, dxsum_scale=0.5,      # noqa: E731
                                     drop=(o.get("drop_p", 0.0), o.get("drop_key", 0)))
    if case["facts"]["rc"]:
        _einval(call)
        return {}, {}
    call()
    got = dict(dx=dx, dgamma=dg, dbeta=db)
    if dx16 is not None:
        got["dx16"] = dx16
    if dxsum is not None:
        got["dxsum"] = dxsum
    extra = {}
    if o.get("drop_p", 0.0) > 0:
        torch.cuda.synchronize()
        keep = (dx16 != 0).cpu()
        _keep_rate(case, keep, torch.ones_like(keep))
        extra["keep"] = keep
    return got, extra


def run_col_reduce(case, inp, bands):
    ops, s, o = _ops(), case["shape"], case["options"]
    M, C, mode = s["M"], s["C"], o.get("mode", 0)
    off = 0 if case["aligned"] else 1

    def launch(i):
        x, y, mask = _dev(i["x"], off), _dev(i["y"]), _dev(i["rowmask"])
        out0 = bands.out((C,), torch.float64, init=0.0)
        out1 = bands.out((C,), torch.float64, init=0.0) if mode else None
        ops.col_reduce(x[:, :C], out0, out1, None if y is None else y[:, :C], mask, mode)
        return dict(out0=out0, out1=out1) if mode else dict(out0=out0)

    # small integers: the sums must be exact in all three modes
    ints = R.make_inputs(dict(case, options=dict(o, ints=True)))
    got = launch(ints)
    ref = R.reference(case, ints)
    torch.cuda.synchronize()
    for k, t in got.items():
        assert torch.equal(t.cpu(), ref[k].ref), (case["id"], k, "integer sums are not exact")
    return launch(inp), {}


def run_f64_to_f32_add(case, inp, bands):
    dst = bands.out((case["shape"]["n"],), init=inp["dst"])
    _ops().f64_to_f32_add(_dev(inp["src"]), dst, inp["scale"])
    return dict(dst=dst), {}


def run_bn_act_fwd(case, inp, bands):
    ops, s, o = _ops(), case["shape"], case["options"]
    M, C = s["M"], s["C"]
    z = _dev(inp["z"], 0 if case["aligned"] else 1)
    y = bands.out((M, C), TDT[case["dtypes"].get("y", "f32")])
    mean, rstd = bands.out((C,)), bands.out((C,))
    rm, rv = bands.out((C,), init=inp["rmean"]), bands.out((C,), init=inp["rvar"])
    ops.bn_act_fwd(z, _dev(inp["stats"]), _dev(inp["g"]), _dev(inp["b"]), rm, rv, mean, rstd, y, inp["eps"], inp["momentum"],
                   o.get("training", True), o.get("act", R.ACT_NONE))
    return dict(y=y, mean=mean, rstd=rstd, running_mean=rm, running_var=rv), {}


def run_bn_act_bwd_a(case, inp, bands):
    ops, s, o = _ops(), case["shape"], case["options"]
    from a3t_amd import _lib
    M, C = s["M"], s["C"]
    dy, z, mean, rstd, g, b = (_dev(inp[k]) for k in ("dy", "z", "mean", "rstd", "g", "b"))
    sums = bands.out((2 * C,), torch.float64, init=0.0)
    _lib.check(_lib.load().a3t_bn_act_bwd_a(ops._ptr(dy), ops._dt(dy), ops._ptr(z), ops._ptr(mean), ops._ptr(rstd), ops._ptr(g), ops._ptr(b),
                                            ops._ptr(sums), M, C, o.get("act", R.ACT_NONE), ops._stream()), "bn_bwd_a")
    return dict(sums=sums), {}


def run_bn_act_bwd_b(case, inp, bands):
    ops, s, o = _ops(), case["shape"], case["options"]
    from a3t_amd import _lib
    M, C = s["M"], s["C"]
    dy, z, mean, rstd, g, b, sums = (_dev(inp[k]) for k in ("dy", "z", "mean", "rstd", "g", "b", "sums"))
    dz = bands.out((M, C))
    dg, db = bands.out((C,), init=inp["dgamma0"]), bands.out((C,), init=inp["dbeta0"])
    _lib.check(_lib.load().a3t_bn_act_bwd_b(ops._ptr(dy), ops._dt(dy), ops._ptr(z), ops._ptr(mean), ops._ptr(rstd), ops._ptr(g), ops._ptr(b),
                                            ops._ptr(sums), ops._ptr(dz), ops._ptr(dg), ops._ptr(db), M, C,
                                            int(o.get("training", True)), o.get("act", R.ACT_NONE), ops._stream()), "bn_bwd_b")
    return dict(dz=dz, dgamma=dg, dbeta=db), {}


def run_glu_dwconv_fwd(case, inp, bands):
    ops, s, o, dt = _ops(), case["shape"], case["options"], case["dtypes"]
    B, T, C, K = s["B"], s["T"], s["C"], s["K"]
    g, w, bias = _dev(inp["g"]), _dev(inp["w"]), _dev(inp["bias"])
    glu = bands.out((B * T, C), TDT[dt.get("glu", "f32")])
    z = bands.out((B * T, C))
    if case["facts"]["rc"]:
        _einval(lambda: ops.glu_dwconv_fwd(g, w, bias, glu, z, T))
        return {}, {}
    if not o.get("ragged"):
        ops.glu_dwconv_fwd(g, w, bias, glu, z, T)
        return dict(glu=glu, z=z), {}
    ops.glu_dwconv_fwd_ragged(g, w, bias, glu, z, _dev(inp["lens"]), B, T)
    for bb, n in enumerate(o["lens"]):      # bit for bit the dense kernel on each row alone (K decides the instantiation)
        if n:
            dense = R.expected_path("glu_dwconv_fwd", dict(B=1, T=n, C=C, K=K))[1]["kernels"]
            assert _same_instantiation(dense, case["facts"]["kernels"])
            g1, z1 = bands.out((n, C)), bands.out((n, C))
            ops.glu_dwconv_fwd(g[bb * T:bb * T + n], w, bias, g1, z1, n)
            assert torch.equal(g1, glu[bb * T:bb * T + n]) and torch.equal(z1, z[bb * T:bb * T + n]), (case["id"], bb, n)
    return dict(glu=glu, z=z), {}


def run_glu_dwconv_bwd(case, inp, bands):
    ops, s, o, dt = _ops(), case["shape"], case["options"], case["dtypes"]
    B, T, C, K = s["B"], s["T"], s["C"], s["K"]
    dz, g, glu, w = _dev(inp["dz"]), _dev(inp["g"]), _dev(inp["glu"]), _dev(inp["w"])
    dg = bands.out((B * T, 2 * C), TDT[dt.get("dg", "f32")])
    dW, db = bands.out((C, K), init=0.0), bands.out((C,), init=0.0)
    dgsum = bands.out((2 * C,), init=0.0) if o.get("dgsum") else None
    if case["facts"]["rc"]:
        _einval(lambda: ops.glu_dwconv_bwd(dz, g, glu, w, dg, dW, db, T, dgsum=dgsum))
        return {}, {}
    ops.glu_dwconv_bwd(dz, g, glu, w, dg, dW, db, T, dgsum=dgsum)
    got = dict(dg=dg, dW=dW, dbias=db)
    if dgsum is not None:
        got["dgsum"] = dgsum
    return got, {}


def run_add_pos_bias(case, inp, bands):
    s = case["shape"]
    qkv = _dev(inp["qkv"])
    qu, qv = bands.out((s["M"], s["d"]), qkv.dtype), bands.out((s["M"], s["d"]), qkv.dtype)
    _ops().add_pos_bias(qkv, _dev(inp["u"]), _dev(inp["v"]), qu, qv)
    return dict(qu=qu, qv=qv), {}


def run_add_pos_bias_bwd(case, inp, bands):
    s = case["shape"]
    dqu, dqv = _dev(inp["dqu"]), _dev(inp["dqv"])
    dqkv = bands.out((s["M"], 3 * s["d"]), dqu.dtype)
    _ops().add_pos_bias_bwd(dqu, dqv, dqkv)
    torch.cuda.synchronize()
    assert bool((dqkv[:, s["d"]:] == SENT).all()), "the k / v columns of dqkv were written"
    return dict(dq=dqkv[:, :s["d"]]), {}


def run_relpos_softmax_fwd(case, inp, bands):
    ops, s, o, dt = _ops(), case["shape"], case["options"], case["dtypes"]
    B, H, T = s["B"], s["H"], s["T"]
    ac, bd = _dev(inp["ac"]), _dev(inp["bd"])
    probs = bands.out((B, H, T, T), TDT[dt.get("p", "f32")])
    if o.get("ragged"):
        ops.relpos_softmax_fwd_ragged(ac, bd, _dev(inp["lens"]), probs, B, H, T, inp["scale"])
        for b, n in enumerate(o["lens"]):      # bit for bit the dense kernel on each row alone, where T = n takes the same kernel
            if n and _same_instantiation(R.expected_path("relpos_softmax_fwd", dict(B=1, H=H, T=n))[1]["kernels"], case["facts"]["kernels"]):
                p1 = bands.out((1, H, n, n))
                ops.relpos_softmax_fwd(ac[b:b + 1, :, :n, :n].contiguous(), bd[b:b + 1, :, :n, :n].contiguous(),
                                       torch.ones(1, n, dtype=torch.uint8, device=DEV), p1, 1, H, n, inp["scale"])
                assert torch.equal(p1[0], probs[b, :, :n, :n]), (case["id"], b, n)
        return dict(probs=probs), {}
    km = _dev(inp["keymask"])
    if o.get("drop_p", 0.0) > 0:
        pdrop = bands.out((B, H, T, T), probs.dtype)
        ops.relpos_softmax_fwd(ac, bd, km, probs, B, H, T, inp["scale"], probs_drop=pdrop, drop=(o["drop_p"], o["drop_key"]))
        torch.cuda.synchronize()
        keep = (pdrop != 0).cpu()
        _keep_rate(case, keep, R.reference(case, inp, torch.ones_like(keep))["probs"].ref > 1e-20)
        return dict(probs=probs, probs_drop=pdrop), dict(keep=keep)
    ops.relpos_softmax_fwd(ac, bd, km, probs, B, H, T, inp["scale"])
    return dict(probs=probs), {}


def _kernel_keep_mask(B, H, T, p, key, dtype):
    """The keep mask the kernels derive from (key, element index): read off a forward over uniform scores, whose probabilities are
    non-zero everywhere."""
    zero = torch.zeros(B, H, T, T, dtype=dtype, device=DEV)
    probs, pdrop = torch.empty_like(zero), torch.empty_like(zero)
    _ops().relpos_softmax_fwd(zero, zero, torch.ones(B, T, dtype=torch.uint8, device=DEV), probs, B, H, T, 1.0, probs_drop=pdrop,
                              drop=(p, key))
    torch.cuda.synchronize()
    return (pdrop != 0).cpu()


def run_relpos_softmax_bwd(case, inp, bands):
    ops, s, o, dt = _ops(), case["shape"], case["options"], case["dtypes"]
    B, H, T = s["B"], s["H"], s["T"]
    odt = TDT[dt.get("o", "f32")]
    probs, rowscale = _dev(inp["probs"]), _dev(inp["rowscale"])
    p, key, hm = o.get("drop_p", 0.0), o.get("drop_key", 0), bool(o.get("head_major"))
    dprobs = bands.out((B, H, T, T), inp["dprobs"].dtype, init=inp["dprobs"])
    ds = dprobs if o.get("inplace") else bands.out((B, H, T, T), odt)
    dbd = bands.out((H, B, T, T) if hm else (B, H, T, T), odt, init=7.0)
    if case["facts"]["rc"]:
        _einval(lambda: ops.relpos_softmax_bwd(probs, dprobs, ds, dbd, B, H, T, inp["scale"], drop_p=p, dbd_head_major=hm, drop_key=key,
                                               rowscale=rowscale))
        return {}, {}
    extra, pdrop = {}, None
    if p > 0:
        # stored mask: any mask will do, so a host-made one; regenerated mask: the kernels' own for this key
        if o.get("stored_mask"):
            keep = torch.rand(B, H, T, T, generator=torch.Generator().manual_seed(key)) >= p
        else:
            keep = _kernel_keep_mask(B, H, T, p, key, probs.dtype)
            _keep_rate(case, keep, torch.ones_like(keep))
        pdrop = _dev((inp["probs"].double() * keep / (1.0 - p)).to(probs.dtype))
        # a probability that is exactly 0 reads as dropped; it contributes nothing either way
        extra["keep"] = keep
    if p > 0 and not o.get("stored_mask"):
        ops.relpos_softmax_bwd(probs, dprobs, ds, dbd, B, H, T, inp["scale"], drop_p=p, dbd_head_major=hm, drop_key=key, rowscale=rowscale)
        ds2 = bands.out((B, H, T, T), odt)
        dbd2 = bands.out(tuple(dbd.shape), odt, init=7.0)
        ops.relpos_softmax_bwd(probs, dprobs, ds2, dbd2, B, H, T, inp["scale"], probs_drop=pdrop, drop_p=p, dbd_head_major=hm,
                               rowscale=rowscale)
        assert torch.equal(ds, ds2) and torch.equal(dbd, dbd2), "regenerated-mask backward differs from the stored-mask one"
    else:
        ops.relpos_softmax_bwd(probs, dprobs, ds, dbd, B, H, T, inp["scale"], probs_drop=pdrop, drop_p=p, dbd_head_major=hm,
                               rowscale=rowscale)
    return dict(ds=ds, dbd=dbd), extra


RUN = {"ln_fwd": run_ln_fwd, "ln_bwd": run_ln_bwd, "col_reduce": run_col_reduce, "f64_to_f32_add": run_f64_to_f32_add,
       "bn_act_fwd": run_bn_act_fwd, "bn_act_bwd_a": run_bn_act_bwd_a, "bn_act_bwd_b": run_bn_act_bwd_b,
       "glu_dwconv_fwd": run_glu_dwconv_fwd, "glu_dwconv_bwd": run_glu_dwconv_bwd, "add_pos_bias": run_add_pos_bias,
       "add_pos_bias_bwd": run_add_pos_bias_bwd, "relpos_softmax_fwd": run_relpos_softmax_fwd,
       "relpos_softmax_bwd": run_relpos_softmax_bwd}


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_rowkernel_path(cid):
    case = R.CASE_BY_ID[cid]
    assert case["predicted"] == case["label"]
    inp = R.make_inputs(case)
    bands = Bands()
    got, extra = RUN[case["op"]](case, inp, bands)
    bands.intact()
    if case["facts"]["rc"]:
        print(f"RATIO {case['label']!r} [{cid}]: refused with A3T_EINVAL")
        return
    ref = R.reference(case, inp, extra.get("keep"))
    _compare(case, got, ref, R.case_intrinsic_error(case, ref))
