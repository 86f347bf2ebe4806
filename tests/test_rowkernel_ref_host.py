"""Host checks of tests/rowkernel_ref.py: every float64 reference against torch autograd in float64 (1e-12 of the tensor's largest
magnitude), the ragged references row by row against the dense ones, the path predictor against the case table, and the case table
against the kernel instantiations the build reports.  No GPU."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import rowkernel_ref as R
from oracle import a3t_oracle as O

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _r(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


def _same(got, exp, what=""):
    tol = 1e-12 * max(1.0, float(exp.abs().max()))
    err = float((got - exp).abs().max()) if got.numel() else 0.0
    assert got.shape == exp.shape and err <= tol, (what, err, tol)


def _mag_ok(out):
    assert bool((out.mag >= out.ref.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("M,D", [(7, 40), (5, 384), (3, 1000)])
def test_layernorm_references(M, D):
    x, g, b = _r(M, D, seed=1).requires_grad_(True), (1 + 0.2 * _r(D, seed=2)).requires_grad_(True), _r(D, seed=3).requires_grad_(True)
    y = F.layer_norm(x, (D,), g, b, 1e-5)
    fw = R.ref_layernorm_fwd(x.detach(), g.detach(), b.detach(), 1e-5)
    _same(fw["y"].ref, y.detach(), "y")
    _same(fw["mean"].ref, x.detach().mean(1))
    _same(fw["rstd"].ref, 1 / torch.sqrt(x.detach().var(1, unbiased=False) + 1e-5))
    dy, dres = _r(M, D, seed=4), _r(M, D, seed=5)
    y.backward(dy)
    bw = R.ref_layernorm_bwd(dy, x.detach(), g.detach(), fw["mean"].ref, fw["rstd"].ref, dres, 0.5)
    _same(bw["dx"].ref, x.grad + dres, "dx")
    _same(bw["dgamma"].ref, g.grad, "dgamma")
    _same(bw["dbeta"].ref, b.grad, "dbeta")
    _same(bw["dxsum"].ref, 0.5 * (x.grad + dres).sum(0), "dxsum")
    _same(bw["dx16"].ref, bw["dx"].ref)
    _same(R.ref_layernorm_bwd(dy, x.detach(), g.detach(), fw["mean"].ref, fw["rstd"].ref)["dx"].ref, x.grad, "no dres")
    # the dropout-carrying outputs: dx itself is not dropped
    keep = (_r(M, D, seed=6) > -1.0).to(F64)
    dr = R.ref_layernorm_bwd(dy, x.detach(), g.detach(), fw["mean"].ref, fw["rstd"].ref, dres, 0.5, keep, 0.25)
    _same(dr["dx"].ref, x.grad + dres)
    _same(dr["dx16"].ref, keep * (x.grad + dres) / 0.75)
    _same(dr["dxsum"].ref, 0.5 * (keep * (x.grad + dres) / 0.75).sum(0))
    for o in list(fw.values()) + list(bw.values()):
        _mag_ok(o)


def test_layernorm_ragged_reference_is_the_dense_one_row_by_row():
    B, T, D, lens = 5, 70, 40, R.RAGGED_LENS_70
    x, g, b = _r(B * T, D, seed=1), _r(D, seed=2), _r(D, seed=3)
    xn = x.clone()
    for bb, n in enumerate(lens):
        xn[bb * T + n:(bb + 1) * T] = float("nan")
    rg = R.ref_layernorm_fwd_ragged(xn, g, b, 1e-5, lens, B, T)
    for bb, n in enumerate(lens):
        for k in ("y", "mean", "rstd"):
            assert not bool(rg[k].ref[bb * T + n:(bb + 1) * T].any())
            if n:
                assert torch.equal(rg[k].ref[bb * T:bb * T + n], R.ref_layernorm_fwd(x[bb * T:bb * T + n], g, b, 1e-5)[k].ref)


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_SWISH, R.ACT_TANH])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("M", [2, 23])
def test_batchnorm_references(act, training, M):
    C = 12
    z = _r(M, C, seed=1).requires_grad_(True)
    g, b = (1 + 0.2 * _r(C, seed=2)).requires_grad_(True), _r(C, seed=3).requires_grad_(True)
    rm, rv = _r(C, seed=4), 1 + 0.1 * _r(C, seed=5).abs()
    trm, trv = rm.clone(), rv.clone()
    bn = F.batch_norm(z, trm, trv, g, b, training, 0.1, 1e-5)
    y = bn * torch.sigmoid(bn) if act == R.ACT_SWISH else (torch.tanh(bn) if act == R.ACT_TANH else bn)
    zd = z.detach()
    stats = torch.cat([zd.sum(0), (zd * zd).sum(0)])
    fw = R.ref_bn_act_fwd(zd, stats, g.detach(), b.detach(), rm, rv, 1e-5, 0.1, training, act)
    _same(fw["y"].ref, y.detach(), "y")
    _same(fw["running_mean"].ref, trm, "running mean")
    _same(fw["running_var"].ref, trv, "running var (unbiased)")
    if training and M == 23:
        assert float((trv - (0.9 * rv + 0.1 * zd.var(0, unbiased=True))).abs().max()) < 1e-12
    dy = _r(M, C, seed=6)
    y.backward(dy)
    a = R.ref_bn_act_bwd_a(dy, zd, fw["mean"].ref, fw["rstd"].ref, g.detach(), b.detach(), act)
    _same(a["sums"].ref[C:], g.grad, "sum d zhat = dgamma")
    _same(a["sums"].ref[:C], b.grad, "sum d = dbeta")
    dg0, db0 = _r(C, seed=7), _r(C, seed=8)
    bb = R.ref_bn_act_bwd_b(dy, zd, fw["mean"].ref, fw["rstd"].ref, g.detach(), b.detach(), a["sums"].ref, dg0, db0, training, act)
    _same(bb["dz"].ref, z.grad, "dz")
    _same(bb["dgamma"].ref, dg0 + g.grad)
    _same(bb["dbeta"].ref, db0 + b.grad)
    for o in (fw["y"], a["sums"], bb["dz"]):
        _mag_ok(o)


def test_col_reduce_reference():
    M, C = 37, 9
    x, y = _r(M, C, seed=1), _r(M, C, seed=2)
    mask = (torch.arange(M) % 3 != 0).to(torch.uint8)
    assert "out1" not in R.ref_col_reduce(x, 0)
    _same(R.ref_col_reduce(x, 0)["out0"].ref, x.sum(0))
    _same(R.ref_col_reduce(x, 1)["out1"].ref, (x * x).sum(0))
    r = R.ref_col_reduce(x, 2, y, mask)
    _same(r["out0"].ref, x[mask.bool()].sum(0))
    _same(r["out1"].ref, (x * y)[mask.bool()].sum(0))
    # `ld`: the reference sees the [M][C] view of a wider buffer
    wide = _r(M, C + 3, seed=3)
    _same(R.ref_col_reduce(wide[:, :C], 1)["out1"].ref, (wide[:, :C] ** 2).sum(0))


@pytest.mark.parametrize("B,T,C,K", [(2, 9, 5, 7), (1, 1, 3, 31), (3, 15, 4, 31), (2, 70, 3, 5), (2, 12, 3, 1)])
def test_glu_dwconv_references(B, T, C, K):
    g = _r(B * T, 2 * C, seed=1).requires_grad_(True)
    w, bias = _r(C, K, seed=2).requires_grad_(True), _r(C, seed=3).requires_grad_(True)
    glu = F.glu(g.view(B, T, 2 * C).transpose(1, 2), dim=1)
    z = F.conv1d(glu, w.view(C, 1, K), bias, padding=(K - 1) // 2, groups=C).transpose(1, 2)
    fw = R.ref_glu_dwconv_fwd(g.detach(), w.detach(), bias.detach(), B, T)
    _same(fw["glu"].ref, glu.detach().transpose(1, 2).reshape(B * T, C), "glu")
    _same(fw["z"].ref, z.detach().reshape(B * T, C), "z")
    dz = _r(B * T, C, seed=4)
    z.backward(dz.view(B, T, C))
    bw = R.ref_glu_dwconv_bwd(dz, g.detach(), fw["glu"].ref, w.detach(), B, T)
    _same(bw["dg"].ref, g.grad, "dg")
    _same(bw["dW"].ref, w.grad, "dW")
    _same(bw["dbias"].ref, bias.grad, "dbias")
    _same(bw["dgsum"].ref[:C], g.grad[:, :C].sum(0), "dgsum a")
    _same(bw["dgsum"].ref[C:], g.grad[:, C:].sum(0), "dgsum b")
    for o in (fw["z"], bw["dg"], bw["dW"], bw["dgsum"]):
        _mag_ok(o)


def test_glu_dwconv_ragged_reference_is_the_dense_one_row_by_row():
    B, T, C, K, lens = 5, 70, 6, 15, R.RAGGED_LENS_70
    g, w, bias = _r(B * T, 2 * C, seed=1), _r(C, K, seed=2), _r(C, seed=3)
    gn = g.clone()
    for b, n in enumerate(lens):
        gn[b * T + n:(b + 1) * T] = float("nan")
    rg = R.ref_glu_dwconv_fwd_ragged(gn, w, bias, lens, B, T)
    for b, n in enumerate(lens):
        for k in ("glu", "z"):
            assert not bool(rg[k].ref[b * T + n:(b + 1) * T].any())
            if n:
                assert torch.equal(rg[k].ref[b * T:b * T + n], R.ref_glu_dwconv_fwd(g[b * T:b * T + n], w, bias, 1, n)[k].ref)


def test_add_pos_bias_references():
    M, d = 7, 6
    qkv, u, v = _r(M, 3 * d, seed=1).requires_grad_(True), _r(d, seed=2), _r(d, seed=3)
    qu, qv = qkv[:, :d] + u, qkv[:, :d] + v
    r = R.ref_add_pos_bias(qkv.detach(), u, v, d)
    _same(r["qu"].ref, qu.detach())
    _same(r["qv"].ref, qv.detach())
    a, b = _r(M, d, seed=4), _r(M, d, seed=5)
    (qu * a + qv * b).sum().backward()
    _same(R.ref_add_pos_bias_bwd(a, b)["dq"].ref, qkv.grad[:, :d])
    assert not bool(qkv.grad[:, d:].any())


@pytest.mark.parametrize("T", [1, 2, 9, 37])
def test_rel_shift_gather_is_the_legacy_reshape(T):
    bd = _r(2, 3, T, T, seed=T)
    assert torch.equal(R.rel_shift_gather(bd), O.rel_shift_legacy(bd))
    idx = R.rel_shift_index(T)
    hit = idx[idx >= 0]
    # compact dBD: every element the scores read is hit exactly once; the rest is exactly BD[0][0..T-2]
    counts = torch.bincount(hit, minlength=T * T)
    assert int(counts.max()) <= 1
    assert torch.equal(torch.nonzero(counts == 0).flatten(), torch.arange(T - 1))
    assert int((idx < 0).sum()) == T - 1


@pytest.mark.parametrize("T", [5, 37])
def test_relpos_softmax_references(T):
    B, H, scale = 3, 2, 0.3
    ac, bd = _r(B, H, T, T, seed=1, scale=3).requires_grad_(True), _r(B, H, T, T, seed=2, scale=3).requires_grad_(True)
    km = torch.ones(B, T, dtype=torch.uint8)
    km[1, T // 2:] = 0
    km[2] = 0
    m = (km == 0)[:, None, None, :]
    s = (ac + O.rel_shift_legacy(bd)) * scale
    pr = torch.softmax(s.masked_fill(m, float(torch.finfo(torch.float32).min)), dim=-1).masked_fill(m, 0.0)
    fw = R.ref_relpos_softmax_fwd(ac.detach(), bd.detach(), km, scale)
    _same(fw["probs"].ref, pr.detach(), "probs")
    assert not bool(fw["probs"].ref[2].any())          # a whole utterance padded -> zeros
    dp = _r(B, H, T, T, seed=3)
    pr.backward(dp)
    dbd0 = torch.full((B, H, T, T), 7.0, dtype=F64)
    bw = R.ref_relpos_softmax_bwd(pr.detach(), dp, scale, dbd0)
    _same(bw["ds"].ref, ac.grad, "ds")
    _same(bw["dbd"].ref, bd.grad, "dbd")                # autograd leaves BD[0][0..T-2] at 0 as well
    assert not bool(bw["dbd"].ref[..., 0, :T - 1].any())
    hm = R.ref_relpos_softmax_bwd(pr.detach(), dp, scale, dbd0, head_major=True)
    assert torch.equal(hm["dbd"].ref, bw["dbd"].ref.transpose(0, 1))
    # rowscale: un-normalised probabilities times their normaliser
    rs = 0.5 + _r(B * H * T, seed=4).abs()
    un = R.ref_relpos_softmax_bwd(pr.detach() / rs.view(B, H, T, 1), dp, scale, dbd0, rowscale=rs)
    _same(un["ds"].ref, ac.grad, "rowscale")
    # dropout: d probs = keep * d probs_drop / (1 - p)
    keep = (_r(B, H, T, T, seed=5) > -0.8).to(F64)
    ac.grad = bd.grad = None
    pr2 = torch.softmax(((ac + O.rel_shift_legacy(bd)) * scale).masked_fill(m, float(torch.finfo(torch.float32).min)), dim=-1).masked_fill(m, 0.0)
    pd = pr2 * keep / 0.8
    pd.backward(dp)
    fd = R.ref_relpos_softmax_fwd(ac.detach(), bd.detach(), km, scale, keep, 0.2)
    _same(fd["probs_drop"].ref, pd.detach(), "probs_drop")
    bd_ = R.ref_relpos_softmax_bwd(pr2.detach(), dp, scale, dbd0, keep, 0.2)
    _same(bd_["ds"].ref, ac.grad, "ds under dropout")
    _same(bd_["dbd"].ref, bd.grad, "dbd under dropout")
    _mag_ok(fw["probs"])
    _mag_ok(bw["ds"])


def test_relpos_softmax_ragged_reference_is_the_dense_one_row_by_row():
    B, H, T, lens = 5, 2, 70, R.RAGGED_LENS_70
    ac, bd = _r(B, H, T, T, seed=1), _r(B, H, T, T, seed=2)
    rg = R.ref_relpos_softmax_fwd_ragged(ac, bd, lens, 0.3)["probs"].ref
    for b, n in enumerate(lens):
        assert not bool(rg[b, :, n:, :].any()) and not bool(rg[b, :, :, n:].any())
        if n:
            alone = R.ref_relpos_softmax_fwd(ac[b:b + 1, :, :n, :n].contiguous(), bd[b:b + 1, :, :n, :n].contiguous(),
                                             torch.ones(1, n, dtype=torch.uint8), 0.3)["probs"].ref
            assert torch.equal(rg[b, :, :n, :n], alone[0])
            _same(alone.sum(-1), torch.ones(1, H, n, dtype=F64))


def test_bound_and_helpers():
    o = R.Out(torch.tensor([2.0], dtype=F64), torch.tensor([4.0], dtype=F64), True)
    assert float(R.bound(o, 10, "f32")) == 18 * R.EPS * 4.0
    assert float(R.bound(o, 10, "f32", 1e-7)) == (18 * R.EPS + 2e-7) * 4.0
    assert float(R.bound(o, 10, "bf16")) == 18 * R.EPS * 4.0 + 2.0 ** -8 * 2.0
    assert float(R.bound(o, 10, "f64", 1e-7)) == 10 * R.EPS * 4.0
    assert R.demangle("_Z19ln_bwd_row64_kernelILi3ELb1EEvPKviPKfS3_S3_S3_S3_PfPtS4_S4_S4_fiijfj") == ("ln_bwd_row64_kernel", (3, True))
    assert R.demangle("_Z13ln_bwd_kernelILi24EEvPKviPKfS3_S3_S3_S3_PfPtS4_S4_S4_fii") == ("ln_bwd_kernel", (24,))
    assert R.demangle("_Z17col_reduce_kernelPKviPKfPKhPdS5_iilii") == ("col_reduce_kernel", ())
    lo, hi = R.keep_rate_interval(10000, 0.1)
    assert lo < 9000 < hi and hi - lo == pytest.approx(10 * (10000 * 0.9 * 0.1) ** 0.5, rel=1e-3)
    assert 0.0 < R.intrinsic_error("sigmoid", _r(1000, seed=1)) < 1e-6


def test_predictor_launch_facts():
    """The facts behind the labels the issue is about: which loops wrap, and how unevenly."""
    f = R.CASE_BY_ID["ln_bwd_pipeline"]["facts"]
    M = R.CASE_BY_ID["ln_bwd_pipeline"]["shape"]["M"]
    assert (f["grid"], f["trips"], f["trips_min"]) == (512, 2, 1) and M % 8 and (M - 4096) % 8       # some waves two rows, some one
    f = R.CASE_BY_ID["ln_bwd_wrap"]["facts"]
    assert (f["grid"], f["trips"], f["trips_min"]) == (2048, 2, 1)
    f = R.CASE_BY_ID["dw_bwd_vec_tpb_k7"]["facts"]
    assert (f["grid"], f["tiles_per_block"], f["trips_min"]) == ((1, 640), 2, 1)
    f = R.CASE_BY_ID["dw_bwd_tpb_k31"]["facts"]
    assert (f["grid"], f["tiles_per_block"], f["trips_min"]) == ((1, 1024), 2, 1)
    assert R.expected_path("glu_dwconv_bwd", dict(B=2, T=1120, C=384, K=31))[1]["tiles_per_block"] == 1    # the largest older shape
    for cid in ("bn_fwd_vec_wrap", "bn_fwd_gen_wrap", "bn_bwdb_vec_wrap", "bn_bwdb_gen_wrap", "add_pos_bias_vec_wrap",
                "add_pos_bias_f32_wrap", "add_pos_bias_bwd_vec_wrap", "add_pos_bias_bwd_f32_wrap"):
        c = R.CASE_BY_ID[cid]
        assert c["facts"]["grid"] == 4096 and c["facts"]["trips"] == 2, cid
        width = c["shape"].get("C", c["shape"].get("d"))
        assert width & (width - 1), cid                    # not a power of two: the column of a wrapped index is not a bit mask
    # the smallest size over the cap: one row less stays under it
    for cid in ("bn_fwd_vec_wrap", "bn_fwd_gen_wrap", "add_pos_bias_vec_wrap", "add_pos_bias_f32_wrap"):
        c = R.CASE_BY_ID[cid]
        less = dict(c["shape"], M=c["shape"]["M"] - 1)
        assert R.expected_path(c["op"], less, c["dtypes"], c["aligned"], c["options"])[1]["trips"] == 1, cid
    for c in R.CASES:
        if c["options"].get("ragged"):
            lens, T = c["options"]["lens"], c["shape"].get("T", c["options"].get("T"))
            assert {0, 1, T, 64, 65} <= set(lens), c["id"]


def test_every_case_reaches_its_label():
    for c in R.CASES:
        assert c["predicted"] == c["label"], c["id"]
        assert (c["L"] is None) == (c["facts"]["rc"] != 0), c["id"]
    assert len({c["id"] for c in R.CASES}) == len(R.CASES)


def test_the_table_reaches_exactly_the_required_labels():
    reached = {c["label"] for c in R.CASES}
    required = set(R.REQUIRED_LABELS)
    assert len(required) == len(R.REQUIRED_LABELS)
    assert sorted(required - reached) == [], "labels without a case"
    assert sorted(reached - required) == [], "cases whose label is not in the contract"


def test_every_built_instantiation_is_claimed_by_a_case():
    path = os.path.join(ROOT, "a3t_amd", "lib", "norm_reduce.resources.json")
    if not os.path.exists(path):
        pytest.skip("library not built by a3t_amd.build in this tree")
    claimed = {k for c in R.CASES for k in c["facts"]["kernels"]}
    unclaimed = [sym for sym in json.load(open(path)) if R.demangle(sym) not in claimed]
    assert unclaimed == []
