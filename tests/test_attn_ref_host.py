"""tests/attn_ref.py checked on the host: the float64 score-gradient reference against autograd, the skew against the adjoint of
the oracle's rel_shift, the restated task walk, the case table's labels for four device sizes, and the error bound against two
fp32 emulations of the kernel's arithmetic (printed: the worst error / bound ratios; `pytest -s` shows them)."""
import math

import pytest
import torch

import attn_ref as A
from oracle import a3t_oracle as O

F64 = torch.float64
CUS = (64, 128, 256, 304)


# ------------------------------------------------------------------------------------------------ 1. reference == autograd
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,H,T,dk", [(3, 2, 40, 32), (2, 3, 24, 64), (1, 1, 56, 96)])
def test_reference_equals_float64_autograd_through_the_scores(B, H, T, dk, mode):
    """softmax -> dropout -> @ v, differentiated through the raw scores (the formula of _exact_bwd in test_gpu_attn_fused.py).
    The reference receives the same numbers in float64: rowscale = 1 / the row sum of |probs|, ctx = the forward's exact output."""
    op = A.make_operands(B, H, T, dk, mode, seed=7 * T + dk + mode)
    d = H * dk
    sc = A.f32(op["scale"])
    e = op["probs"].abs().to(F64)
    valid = (torch.arange(T)[None, :] < torch.tensor(op["lengths"])[:, None])[:, None, None, :].expand(B, H, T, T)
    assert bool((e[~valid] == 0).all()) and bool((e[valid] > 0).all())
    raw = (torch.log(e.clamp_min(1e-300)) / sc).masked_fill(~valid, -1e300).requires_grad_(True)
    pr = torch.softmax(raw * sc, dim=-1).masked_fill(~valid, 0.0)
    keep = A.keep_of(op["probs"], op["drop"], mode)
    dinv = float(A.SK.drop_inv(op["drop"][0])) if mode else 1.0
    v = op["qkv"][:, 2 * d:]
    ctx = ((pr * keep * dinv) @ A.heads(v, B, H, T, dk)).transpose(1, 2).reshape(B * T, d)
    ctx.backward(op["dctx"].to(F64))
    rsum = e.sum(-1)
    rowscale = torch.where(rsum > 0, 1.0 / rsum, torch.zeros_like(rsum))
    o = A.ref_bwd_ds(op["dctx"], ctx.detach(), v, op["probs"], rowscale, op["scale"], op["drop"], mode)
    err = float((o.ref - raw.grad).abs().max())
    assert float(raw.grad.abs().max()) > 1e-3 and err < 1e-12, err
    if B > 2:
        assert not bool(o.ref[2].any())                       # the fully masked batch row
    if mode:
        frac = 1.0 - float(keep.double().mean())
        assert abs(frac - op["drop"][0]) < 0.03, frac
    assert bool((o.mag >= o.ref.abs() * (1 - 1e-12)).all())


def test_inverse_skew_is_the_adjoint_of_the_legacy_rel_shift():
    g = torch.Generator().manual_seed(3)
    for T in (8, 33, 40):
        ds = torch.randn(2, 3, T, T, generator=g, dtype=F64)
        x = torch.zeros(2, 3, T, T, dtype=F64, requires_grad=True)
        (O.rel_shift_legacy(x) * ds).sum().backward()
        got = A.inverse_skew(ds)
        assert torch.equal(got, x.grad)
        assert not bool(got[..., 0, :T - 1].any())
        bits = ds.to(torch.bfloat16)
        assert torch.equal(A.inverse_skew(bits).view(torch.int16), A.inverse_skew(bits.view(torch.int16)))


# ------------------------------------------------------------------------------------------------------------- 2. the walk
WALK_SHAPES = [(3, 2, 32), (5, 3, 168), (7, 2, 200), (33, 2, 264), (29, 2, 328), (130, 2, 168), (19, 3, 328), (32, 2, 1120), (1, 1, 8)]


@pytest.mark.parametrize("cus", (4, 64, 256))
@pytest.mark.parametrize("B,H,T", WALK_SHAPES)
def test_walk_hands_out_every_task_once_in_contiguous_ranges(B, H, T, cus):
    w = A.walk(B, H, T, cus)
    g = w.geometry
    assert sorted(gr.vb for gr in w.groups) == list(range(g.grid))            # xcd_contiguous permutes the range indices
    seen = []
    for gr in w.groups:
        idx = [t.index for t in gr.tasks]
        assert idx == list(range(gr.vb * g.tper, gr.vb * g.tper + len(idx))) and len(idx) <= g.tper
        assert ("idle" in gr.facts) == (not idx)
        seen += idx
    assert sorted(seen) == list(range(g.ntasks))
    # a task's tiles cover the score matrix exactly once
    cover = {}
    for gr in w.groups:
        for t in gr.tasks:
            assert 1 <= t.nt <= A.KT and t.J0 < t.J1 <= T and t.J1 - t.J0 <= 32 * t.nt and 128 * t.qb < T
            key = (t.bh, t.qb, t.J0)
            assert key not in cover
            cover[key] = t.J1
    assert len(cover) == B * H * g.NQB * g.NKC


def test_existing_reference_test_never_walks_and_the_benchmark_shape_walks_eight():
    """The gap this suite closes, written down: at 256 CUs every shape at which an existing test compares a3t_attn_bwd_ds with a
    reference has one task per workgroup.  (test_single_tensor_save_... and test_compact_dbd_... also run (32, 2, 1120), but
    compare the kernel with itself there.)"""
    vs_reference = [(2, 2, 136), (3, 2, 200), (2, 4, 264), (2, 2, 328), (1, 2, 296), (3, 2, 1120)]       # test_score_gradients_...
    vs_itself_small = [(2, 2, 136), (3, 2, 200), (2, 4, 264), (2, 2, 1120), (2, 2, 328), (3, 2, 1120)]
    for B, H, T in vs_reference + vs_itself_small:
        g = A.geometry(B, H, T, 256)
        assert g.tper == 1 and g.ntasks <= 512, (B, H, T, g)
    assert max(A.geometry(B, H, T, 256).ntasks for B, H, T in vs_reference) == 378
    assert A.geometry(32, 2, 1120, 256).tper == 8
    assert A.transition_labels(A.walk(3, 2, 1120, 256)) == set()


@pytest.mark.parametrize("cus", CUS)
def test_case_table_reaches_every_required_label(cus):
    table = A.cases(cus)
    assert tuple(c.name for c in table) == A.CASE_NAMES and len(set(A.CASE_NAMES)) == len(A.CASE_NAMES)
    got = set()
    per = {}
    for c in table:
        w = A.walk(c.B, c.H, c.T, cus)
        assert w.geometry.tper == c.tper >= 2 and w.geometry.grid == 2 * cus, c
        assert c.B >= 3 and c.B * c.H * c.T * c.T * 2 <= 26e6 * max(cus, 256) / 256, c       # bytes of probs
        per[c.name] = A.labels(w)
        got |= per[c.name]
    assert got == set(A.REQUIRED_LABELS), (A.REQUIRED_LABELS - got, got - A.REQUIRED_LABELS)
    tr = lambda n: {x for x in per[n] if x in ("same-block", "new-block", "new-head", "new-batch", "nt1->ntN", "nt1->nt1")}
    assert tr("one_tile") == {"new-head", "new-batch", "nt1->nt1"} and "idle" in per["one_tile"]
    assert sum("idle" in gr.facts for gr in A.walk(table[0].B, table[0].H, 32, cus).groups) == cus - 4       # half of them, less 4
    for dk in A.DKS:
        assert tr(f"strip_5_1_dk{dk}") == {"same-block"} and "wave-past-T" in per[f"strip_5_1_dk{dk}"]
        assert tr(f"cross_5_1_dk{dk}") == {"same-block", "new-block", "new-head", "new-batch", "nt1->ntN"}
        assert "short-last" in per[f"cross_5_1_dk{dk}"]
    for n in (2, 3, 4):
        assert {f"nt{n}", "nt5", "partial-tile"} <= per[f"strip_5_{n}"]
    for n in ("cross_5_5_1_dk64", "cross_5_5_1_dk192", "production"):
        assert tr(n) == {"same-block", "new-block", "new-head", "new-batch", "nt1->ntN"} and "short-last" in per[n]
    by = {c.name: c for c in table}
    assert {c.dbd for c in table} == {"bm", "hm", None}
    assert by["production"].mode == 2 and by["production"].dbd is None and by["production"].dk == 192
    for base in ("strip_5_1_dk64", "tper3_dk192", "cross_5_1_dk64", "cross_5_5_1_dk192"):
        assert by[base].mode == 0 and by[base + "_drop1"].mode == 1 and by[base + "_drop2"].mode == 2
    assert {c.dk for c in table if c.name.startswith("cross_5_1")} == set(A.DKS)


# ------------------------------------------------------------------------------------------------------------ 3. the bound
def test_half_ulp_of_a_bf16_value():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.999, 2.0, -3.0, 0.0, 2.0 ** -20], dtype=F64)
    assert A.hulp_bf16(x).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 0.0, 2.0 ** -28]
    # a correct rounding reaches it: 1 + 2^-8 lies half-way between the neighbours 1 and 1 + 2^-7
    y = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=F64)
    assert float((y.to(torch.float32).to(torch.bfloat16).to(F64) - y).abs()) > 2.0 ** -9 * float(y)


@pytest.mark.parametrize("name", A.CASE_NAMES)
def test_fp32_emulations_of_the_kernel_stay_inside_the_bound(name):
    """The operands of the case (for a 64-CU device: the same shapes with fewer (b, h)), the kernel's arithmetic in fp32 with
    sequential and with pairwise dot products.  Before the bf16 store both stay within HALF of the bound's fp32 term; after it
    within the bound.  (The stored value's ratio comes close to 1 by construction: a bf16 rounding reaches half an ulp.)"""
    case = {c.name: c for c in A.cases(64)}[name]
    op = A.case_operands(case)
    d = case.H * case.dk
    args = (op["dctx"], op["ctx"], op["qkv"][:, 2 * d:], op["probs"], op["rowscale"], op["scale"], op["drop"], case.mode)
    o = A.ref_bwd_ds(*args)
    assert bool(torch.isfinite(o.ref).all()) and float(o.ref.abs().max()) > 1e-3
    assert not bool(o.ref[2].any())
    b = A.bound_ds(o)
    t32 = A.fp32_term(o)
    for pairwise in (False, True):
        x, stored = A.emulate_fp32(*args, pairwise=pairwise)
        r32 = float(((x - o.ref).abs() / t32.clamp_min(1e-300)).max())
        r = float(((stored - o.ref).abs() / b.clamp_min(1e-300)).max())
        print(f"RATIO {name} {'pairwise' if pairwise else 'sequential'}: fp32 error / fp32 term = {r32:.3f}, stored error / bound = {r:.3f}")
        assert r32 <= 0.5, r32
        assert r <= 1.0, r
