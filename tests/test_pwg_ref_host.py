"""tests/pwg_ref.py held against the oracle and torch without a device: the block reference on the packed operands, the layer-path
references, the walk restatement, the case tables and the bound.  tests/test_gpu_pwg_blocks.py then holds the kernels against it."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pwg_f16_ref as R
import pwg_ref as P
from oracle import a3t_oracle as O

F64 = torch.float64
CUS = (64, 256, 304)


def _packed(p, pre):
    from a3t_amd.vocoder import _pack_pwg_block
    wt0, b0, wt1 = _pack_pwg_block(p[pre + "conv.weight"], p[pre + "conv.bias"], p[pre + "conv1x1_aux.weight"],
                                   p[pre + "conv1x1_out.weight"])
    return wt0, b0, wt1, p[pre + "conv1x1_out.bias"].float()


@functools.lru_cache(maxsize=None)
def _operands():
    cw, cb, aw, ow, ob = P.block_params()
    p = {P.PWG_BLOCK + k: v for k, v in zip(("conv.weight", "conv.bias", "conv1x1_aux.weight", "conv1x1_out.weight",
                                             "conv1x1_out.bias"), (cw, cb, aw, ow, ob))}
    return p, _packed(p, P.PWG_BLOCK)


def test_gate_perm_and_tile_list_restate_the_packing():
    from a3t_amd.vocoder import pwg_gate_perm, pwg_tile_list
    assert np.array_equal(P.gate_perm(), pwg_gate_perm())
    ia, ib = P.gate_columns(pwg_gate_perm())
    assert np.array_equal(pwg_gate_perm()[ia.numpy()], np.arange(64)) and np.array_equal(pwg_gate_perm()[ib.numpy()], np.arange(64, 128))
    for W in ((1500, 257, 5), (256, 512, 1), (255,), (513, 513)):
        assert np.array_equal(P.tile_list(W), pwg_tile_list(W, 1))
    assert P.tile_list((0, 0)).shape == (0, 4)


def test_block_ref_equals_the_oracle_taps():
    """Blocks 0 (dilation 1) and 1 (dilation 2) of the generator: block_ref on _pack_pwg_block's operands against the tensors
    pwg_forward taps, all in float64."""
    cfg, state = R.vocoder_state(seed=4)
    p = O.to_torch_state(state, dtype=F64)
    c, z = R.table_inputs(3, B=2)
    c, z = c.double(), z.double()
    taps = {}
    with torch.no_grad():
        O.pwg_forward(p, c, z, cfg, taps=taps)
        w = cfg.aux_context_window
        cu = F.conv1d(F.pad(c, (w, w), mode="replicate"), p["upsample_net.conv_in.weight"]).unsqueeze(1)
        for i, sc in enumerate(cfg.upsample_scales):
            cu = F.conv2d(F.interpolate(cu, scale_factor=(1, sc), mode="nearest"),
                          p[f"upsample_net.upsample.up_layers.{2 * i + 1}.weight"], padding=(0, sc))
        cu = cu.squeeze(1).transpose(1, 2)
        x = F.conv1d(z, p["first_conv.weight"], p["first_conv.bias"]).transpose(1, 2)
    B, Tw, _ = x.shape
    zero = torch.zeros(B, Tw, 64, dtype=F64)
    for l in range(2):
        x, s, _ = P.block_ref(x, cu, zero, *_packed(p, f"conv_layers.{l}."), 2 ** l, (Tw,) * B)
        assert (x - taps[f"x{l}"].transpose(1, 2)).abs().max() <= 1e-12
        assert (s - taps[f"skip{l}"].transpose(1, 2)).abs().max() <= 1e-12


@pytest.mark.parametrize("case", P.BLOCK_CASES, ids=lambda c: c.name)
def test_block_ref_equals_the_convolution_form_row_by_row(case):
    """block_ref (gathers over the packed operands) against pwg_f16_ref.block (conv1d over the raw parameters, no rounding) in
    float64; a ragged row against the row passed alone.  Padding stays what it was."""
    p, ops_ = _operands()
    p64 = {k: v.double() for k, v in p.items()}
    x, cu, sk = P.case_inputs(case)
    xo, so, absw1 = P.block_ref(x, cu, sk, *ops_, case.dil, case.W)
    assert torch.equal(absw1, ops_[2].double().abs().sum(0))
    for b, n in enumerate(case.W):
        with torch.no_grad():
            xr, s = R.block(p64, P.PWG_BLOCK, x[b, :n].double().t()[None], cu[b, :n].double().t()[None], case.dil, O.PWGConfig(),
                            lambda t: t)
        assert (xo[b, :n] - xr[0].t()).abs().max() <= 1e-12
        assert (so[b, :n] - (sk[b, :n].double() + s[0].t())).abs().max() <= 1e-12
        assert torch.isnan(xo[b, n:]).all() and (so[b, n:] == P.SENTINEL).all()


@pytest.mark.parametrize("case", P.BLOCK_CASES, ids=lambda c: c.name)
def test_cpu_fp32_lies_within_a_quarter_of_the_bound(case):
    """The bound's own premise: the CPU's fp32 evaluation (block_ref in float32) is inside a quarter of the allowance at every
    output, and a second fp32 evaluation in another order (conv1d) inside the allowance."""
    p, ops_ = _operands()
    x, cu, sk = P.case_inputs(case)
    r64 = P.block_ref(x, cu, sk, *ops_, case.dil, case.W)
    r32 = P.block_ref(x, cu, sk, *ops_, case.dil, case.W, dtype=torch.float32)
    ax, as_, Fx, Fs = P.allowance(r64[:2], r32[:2], r64[2], case.W)
    print(f"{case.name}: F x_out {Fx:.2e} skips {Fs:.2e}; gate term x_out {float(ax.max()) - 4 * Fx:.2e} skips {float(as_.max()) - 4 * Fs:.2e}")
    assert 1e-7 < Fx < 2e-6 and 1e-7 < Fs < 2e-6                     # the figures the bound was designed around
    m = P.valid_mask(case.B, case.Tw, case.W)
    assert ((r32[0].double() - r64[0]).abs()[m] <= 0.25 * ax).all() and ((r32[1].double() - r64[1]).abs()[m] <= 0.25 * as_).all()
    for b, n in enumerate(case.W):
        with torch.no_grad():
            xr, s = R.block(p, P.PWG_BLOCK, x[b, :n].t()[None], cu[b, :n].t()[None], case.dil, O.PWGConfig(), lambda t: t)
        assert ((xr[0].t().double() - r64[0][b, :n]).abs() <= ax).all()
        assert (((sk[b, :n] + s[0].t()).double() - r64[1][b, :n]).abs() <= as_).all()


# ------------------------------------------------------------------------------------------------------------ layer path
def test_gate_and_res_skip_refs_equal_torch():
    g = torch.Generator().manual_seed(3)
    y, c = torch.randn(37, 128, generator=g, dtype=F64) * 2, torch.randn(37, 128, generator=g, dtype=F64)
    ref, allow = P.gate_ref(y, c)
    ya, yb = (y + c).split(64, dim=1)
    assert (ref - torch.tanh(ya) * torch.sigmoid(yb)).abs().max() <= 1e-12
    assert allow.shape == ref.shape and float(allow.min()) >= P.R_GATE
    o, x, sk = torch.randn(37, 128, generator=g, dtype=F64), torch.randn(37, 64, generator=g, dtype=F64), torch.randn(37, 64, generator=g, dtype=F64)
    xo, so = P.res_skip_ref(o, x, sk)
    r, s = o.split([64, 64], dim=1)
    assert (xo - (r + x) * math.sqrt(0.5)).abs().max() <= 1e-12 and (so - (sk + s)).abs().max() <= 1e-12


@pytest.mark.parametrize("scale", [1, 3, 4, 5])
def test_upsample_ref_equals_interpolate_and_conv2d(scale):
    g = torch.Generator().manual_seed(scale)
    B, Tin, C = 3, 7, 5
    c, w = torch.randn(B, Tin, C, generator=g, dtype=F64), torch.randn(2 * scale + 1, generator=g, dtype=F64)

    def torch_form(cb):      # cb [1][T][C] -> [1][T * scale][C]
        s = F.interpolate(cb.transpose(1, 2).unsqueeze(1), scale_factor=(1, scale), mode="nearest")
        return F.conv2d(s, w.view(1, 1, 1, -1), padding=(0, scale)).squeeze(1).transpose(1, 2)

    assert (P.upsample_ref(c, w, scale) - torch.cat([torch_form(c[b:b + 1]) for b in range(B)])).abs().max() <= 1e-12
    lens, mul = (3, 0, 1), 2
    cn = c.clone()
    for b, n in enumerate(lens):
        cn[b, n * mul:] = float("nan")
    got = P.upsample_ref(cn, w, scale, lens, mul)
    for b, n in enumerate(lens):
        L = n * mul
        assert (got[b, L * scale:] == 0).all()
        if L:
            assert (got[b, :L * scale] - torch_form(c[b:b + 1, :L])[0]).abs().max() <= 1e-12


def test_padding_and_zero_tail_refs_equal_torch():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 12, 5, generator=g, dtype=F64)

    def pad(t, n, mode):     # t [T][C]
        return F.pad(t.t()[None], (n, n), mode=mode)[0].t()

    for n in (0, 2, 4):
        assert torch.equal(P.replicate_pad_ref(x, n), torch.stack([pad(x[b], n, "replicate") for b in range(3)]))
        assert torch.equal(P.reflect_pad_rows_ref(x, n), torch.stack([pad(x[b], n, "reflect") for b in range(3)]))
    xn = x.clone()
    xn[1, 6:], xn[2] = float("nan"), float("nan")
    y = P.replicate_pad_ref(xn, 4, lens=(12, 6, 0))
    assert torch.equal(y[0], pad(x[0], 4, "replicate")) and torch.equal(y[1, :14], pad(x[1, :6], 4, "replicate")) and (y[2] == 0).all()
    assert torch.equal(y[1, 14:], x[1, 5].expand(6, 5))                      # behind the row: its last frame
    y = P.reflect_pad_rows_ref(xn, 4, lens=(4, 2, 0), mul=3)
    assert torch.equal(y[0], pad(x[0], 4, "reflect")) and torch.equal(y[1, :14], pad(x[1, :6], 4, "reflect")) and (y[2] == 0).all()
    assert torch.isfinite(y).all()
    y = P.reflect_pad_rows_ref(xn, 4, lens=(1, 2, 5), mul=1)                # shorter than the pad: clamped into the row
    assert torch.equal(y[0], x[0, 0].expand(20, 5)) and torch.isnan(y[2, 4:9]).all()
    z = P.zero_tail_ref(xn, (4, 2, 0), 3)
    assert torch.equal(z[0], x[0]) and torch.equal(z[1, :6], x[1, :6]) and (z[1, 6:] == 0).all() and (z[2] == 0).all()


# -------------------------------------------------------------------------------------------------------- walk and cases
def test_walk_restates_the_persistent_loop():
    assert P.walk(5, 8) == [[0], [1], [2], [3], [4]]
    assert P.walk(7, 3) == [[0, 3, 6], [1, 4], [2, 5]]
    for n, cus in ((579, 256), (1, 256), (256, 256), (257, 256)):
        w = P.walk(n, cus)
        assert sorted(t for g in w for t in g) == list(range(n)) and len(w) == min(n, cus)


@pytest.mark.parametrize("case", P.BLOCK_CASES, ids=lambda c: c.name)
def test_block_cases_satisfy_the_tile_contract(case):
    P.check_tile_list(P.tile_list(case.W), case.B, case.Tw, case.W)
    assert (case.B, case.Tw) == (3, 1500) or not case.ragged


def test_block_cases_hold_the_shapes_they_are_for():
    names = {c.name: c for c in P.BLOCK_CASES}
    assert {c.dil for c in P.BLOCK_CASES if c.ragged} == {c.dil for c in P.BLOCK_CASES if not c.ragged and c.Tw == 1500} == {1, 8, 512}
    assert all(c.W == (1500, 257, 5) for c in P.BLOCK_CASES if c.ragged)
    assert names["dense_T255_d8"].Tw == 255 and names["dense_T513_d1"].Tw == 513
    with pytest.raises(AssertionError):
        P.check_tile_list(P.tile_list((1500, 257, 5))[:-1], 3, 1500, (1500, 257, 5))
    with pytest.raises(AssertionError):
        P.check_tile_list(P.tile_list((1500, 300, 5)), 3, 1500, (1500, 257, 5))


@pytest.mark.parametrize("cus", CUS)
def test_walk_cases_make_every_workgroup_walk(cus):
    cases = P.walk_cases(cus)
    assert [c.dil for c in cases] == [1, 512, 1, 512] and [c.ragged for c in cases] == [False, False, True, True]
    for case in cases:
        tiles = P.tile_list(case.W)
        P.check_tile_list(tiles, case.B, case.Tw, case.W)
        n = len(tiles)
        w = P.walk(n, cus)
        most = -(-n // cus)
        assert all(len(g) <= most for g in w) and max(len(g) for g in w) >= 3 and min(len(g) for g in w) >= 2
        assert n % cus != 0                                                # the last set of walkers is partial
        assert P.device_bytes(case) < 512e6
        rows = [[tuple(tiles[t][[0, 2]]) for t in g] for g in w]
        if case.ragged:
            assert len(case.W) == 4 and case.W[2] == 5 and case.W[3] % 256 == 1 and case.W[0] % 256 not in (0, 1)
            nt = [-(-x // 256) for x in case.W]
            assert abs(nt[0] - 0.9 * cus) <= 1 and abs(nt[1] - 0.2 * cus) <= 1 and nt[2] == 1 and abs(nt[3] - 1.2 * cus) <= 2
            assert any(a[0] != b[0] and a[1] != b[1] for g in rows for a, b in zip(g, g[1:]))
        else:
            assert case.B == 3 and case.Tw == 256 * math.ceil(0.75 * cus) + 1
            assert all(g[0][0] != g[1][0] for g in rows)                   # the second tile lies in another row
