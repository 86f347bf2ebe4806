"""Host-side checks of the vocoder's fp16-MFMA compute mode: the CPU restatement with rounding points (tests/pwg_f16_ref.py)
against the oracle's generator, the choice of fp16 over bf16 operands, the weight packer and the constructor's refusals."""
import numpy as np
import pytest
import torch

import pwg_f16_ref as R
from oracle import a3t_oracle as O

# the restatement's own loss on these inputs is 5.9e-4 / 5.7e-4 (RMS) and 8.5e-4 / 1.15e-3 (worst element); the caps are
# about 1.7 x that and keep the helper from silently changing its rounding points
RMS_CAP, WORST_CAP = 1e-3, 2e-3


@pytest.fixture(scope="module")
def runs():
    cfg, state = R.vocoder_state(seed=4)
    p = O.to_torch_state(state)
    out = {}
    for T in (40, 120):
        c, z = R.table_inputs(T)
        with torch.no_grad():
            ref = O.pwg_forward(p, c, z, cfg)
        out[T] = dict(ref=ref, none=R.pwg_forward(p, c, z, cfg, None), f16=R.pwg_forward(p, c, z, cfg, torch.float16),
                      bf16=R.pwg_forward(p, c, z, cfg, torch.bfloat16))
    return out


@pytest.mark.parametrize("T", [40, 120])
def test_restatement_without_rounding_is_the_oracle(runs, T):
    d = float((runs[T]["none"] - runs[T]["ref"]).abs().max())
    print(f"T = {T}: restatement without rounding against pwg_forward: max |diff| {d}")
    assert torch.equal(runs[T]["none"], runs[T]["ref"])


@pytest.mark.parametrize("T", [40, 120])
def test_fp16_rounding_against_the_fp32_oracle(runs, T):
    rms, worst = R.errors(runs[T]["f16"], runs[T]["ref"])
    print(f"T = {T}: fp16 operands: RMS error / RMS {rms:.3e}, worst element / max {worst:.3e}")
    assert rms <= RMS_CAP and worst <= WORST_CAP


@pytest.mark.parametrize("T", [40, 120])
def test_bf16_operands_are_worse_than_fp16(runs, T):
    rms16, worst16 = R.errors(runs[T]["f16"], runs[T]["ref"])
    rmsb, worstb = R.errors(runs[T]["bf16"], runs[T]["ref"])
    print(f"T = {T}: bf16 operands: RMS error / RMS {rmsb:.3e}, worst element / max {worstb:.3e} (fp16: {rms16:.3e}, {worst16:.3e})")
    assert rmsb > rms16 and worstb > worst16


def test_operands_stay_far_inside_the_fp16_range():
    cfg, state = R.vocoder_state(seed=4)
    c, z = R.table_inputs(40)
    stats = {}
    R.pwg_forward(O.to_torch_state(state), c, z, cfg, torch.float16, stats)
    print(f"max |x| {stats['max_x']:.2f}, max |cu| {stats['max_cu']:.2f}")
    assert stats["max_x"] < 100 and stats["max_cu"] < 100


def _check_block_layout(w0, b0, w1, conv_w, conv_b, aux_w, out_w, perm, rnd):
    """w0 [272][128] / b0 / w1 [64][128] against an index formula of the test's own; rnd: the rounding of the weights."""
    for tap in range(3):
        want = rnd(conv_w[:, :, tap])[perm].t()                        # [in][n']
        assert torch.equal(w0[tap * 64:(tap + 1) * 64].float(), want), tap
    assert torch.equal(w0[192:].float(), rnd(aux_w[:, :, 0])[perm].t())
    assert torch.equal(w1.float(), rnd(out_w[:, :, 0]).t())
    assert torch.equal(b0, conv_b[perm])


def test_packer_layout_and_rounding():
    """w0h [272][128]: tap-major K order (k = tap * 64 + in channel | 192 + aux channel), columns in the gate permutation; w1h =
    conv1x1_out.weight^T; dequantised they ARE the permuted fp32 weights rounded to fp16; saturation instead of infinity.
    Second case: the fp32 operands of the fused path (wt0 / b0 / wt1 of a generator) against the same formula without rounding."""
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP, pack_pwg_block_f16, pwg_gate_perm
    rs = np.random.RandomState(11)
    conv_w = torch.from_numpy(rs.standard_normal((128, 64, 3)).astype(np.float32))
    conv_b = torch.from_numpy(rs.standard_normal(128).astype(np.float32))
    aux_w = torch.from_numpy(rs.standard_normal((128, 80, 1)).astype(np.float32))
    out_w = torch.from_numpy(rs.standard_normal((128, 64, 1)).astype(np.float32))
    conv_w[5, 7, 2] = 1e6
    out_w[3, 9, 0] = -1e6
    w0h, b0, w1h = pack_pwg_block_f16(conv_w, conv_b, aux_w, out_w)
    assert w0h.shape == (272, 128) and w0h.dtype == torch.float16 and w0h.is_contiguous()
    assert w1h.shape == (64, 128) and w1h.dtype == torch.float16 and w1h.is_contiguous()
    assert b0.shape == (128,) and b0.dtype == torch.float32
    perm = pwg_gate_perm()
    assert sorted(perm.tolist()) == list(range(128))
    # column n' = 64 * (c // 32) + 32 * half + c % 32 of gate channel c: conv output channel c + 64 * half
    for c in (0, 31, 32, 63):
        for half in (0, 1):
            assert perm[64 * (c // 32) + 32 * half + c % 32] == c + 64 * half
    _check_block_layout(w0h, b0, w1h, conv_w, conv_b, aux_w, out_w, perm, R.rounder(torch.float16))
    assert torch.isfinite(w0h.float()).all() and torch.isfinite(w1h.float()).all()
    n5 = int(np.where(perm == 5)[0][0])
    assert float(w0h[2 * 64 + 7, n5]) == 65504.0 and float(w1h[9, 3]) == -65504.0
    with pytest.raises(ValueError):
        pack_pwg_block_f16(conv_w[:, :32], conv_b, aux_w, out_w)
    cfg, state = R.vocoder_state(seed=4)
    gen = ParallelWaveGANGeneratorHIP(state, device="cpu", fused=True)
    for l in (0, 17):
        blk, (cw, cb, aw, ow) = gen.blocks[l], (torch.as_tensor(np.asarray(state[f"conv_layers.{l}.{k}"]), dtype=torch.float32)
                                                for k in ("conv.weight", "conv.bias", "conv1x1_aux.weight", "conv1x1_out.weight"))
        for name, shape in (("wt0", (272, 128)), ("b0", (128,)), ("wt1", (64, 128))):
            assert blk[name].shape == shape and blk[name].dtype == torch.float32 and blk[name].is_contiguous()
        _check_block_layout(blk["wt0"], blk["b0"], blk["wt1"], cw, cb, aw, ow, perm, lambda t: t)


def test_packer_agrees_with_the_fp32_operands_of_the_fused_path():
    """Same rows, columns and bias order as the wt0 / b0 / wt1 the fp32 fused kernels get."""
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP, pack_pwg_block_f16
    cfg, state = R.vocoder_state(seed=4)
    gen = ParallelWaveGANGeneratorHIP(state, device="cpu", fused=True)
    rnd = R.rounder(torch.float16)
    for l in (0, 17):
        pre = f"conv_layers.{l}."
        w0h, b0, w1h = pack_pwg_block_f16(state[pre + "conv.weight"], state[pre + "conv.bias"], state[pre + "conv1x1_aux.weight"],
                                          state[pre + "conv1x1_out.weight"])
        blk = gen.blocks[l]
        assert torch.equal(w0h.float(), rnd(blk["wt0"])) and torch.equal(b0, blk["b0"]) and torch.equal(w1h.float(), rnd(blk["wt1"]))


def test_new_entry_points_are_exported():
    from a3t_amd import _lib
    assert "a3t_pwg_block_f16" in _lib.EXPORTS and "a3t_cast_f16_sat" in _lib.EXPORTS
    assert len(_lib._SIGS["a3t_pwg_block_f16"]) == 14 and len(_lib._SIGS["a3t_cast_f16_sat"]) == 4


PWG_OPERANDS = ("x", "cu", "wt0", "b0", "wt1", "b1", "g", "skips")
# argument order of the five entry points of the tiled waveform kernels; pointers are named after what they hold
ENTRY_ARGS = {
    "a3t_pwg_block": PWG_OPERANDS + ("B", "Tw", "dil", "stream"),
    "a3t_pwg_block_ragged": PWG_OPERANDS + ("tiles", "ntiles", "B", "Tw", "dil", "stream"),
    "a3t_pwg_block_f16": ("x", "y", "cu", "wt0", "b0", "wt1", "b1", "skips", "tiles", "ntiles", "B", "Tw", "dil", "stream"),
    "a3t_hfg_conv": ("x", "wt0", "b0", "R", "y", "acc", "alpha", "acc_add", "slope", "tiles", "ntiles", "B", "Tw", "C", "taps",
                     "dil", "stream"),
    "a3t_hfg_out": ("x", "wt0", "b0", "y", "slope", "tiles", "ntiles", "B", "Tw", "C", "K", "stream"),
}
DENSE = ("a3t_pwg_block", "a3t_pwg_block_f16", "a3t_hfg_conv", "a3t_hfg_out")
WITH_LIST = ("a3t_pwg_block_ragged", "a3t_pwg_block_f16", "a3t_hfg_conv", "a3t_hfg_out")


def _refusal_rows(tl):
    """(entry, the arguments that differ from a call that would launch); tl: the address of an aligned tile list."""
    rows = []
    for name in WITH_LIST:
        rows += [(name, dict(tiles=tl + 4, ntiles=1)), (name, dict(tiles=tl, ntiles=-1)), (name, dict(tiles=None, ntiles=1))]
    for name, args in ENTRY_ARGS.items():
        rows += [(name, {k: v}) for k in ("B", "Tw", "dil") if k in args for v in (0, -1)]
    # a dense grid of 2^20 x 2^23 tiles, beyond INT_MAX (and Tw + 255 beyond it already)
    rows += [(name, dict(B=1 << 20, Tw=0x7fffffff)) for name in DENSE]
    for name in ("a3t_pwg_block", "a3t_pwg_block_ragged"):
        rows += [(name, {k: None}) for k in PWG_OPERANDS]
    rows.append(("a3t_pwg_block_ragged", dict(tiles=None, ntiles=0)))
    return rows


def test_entry_point_refuses_bad_arguments_on_the_host():
    """Aliasing, misalignment and non-positive sizes are refused before anything is launched (no device needed), and the five
    entry points of the tiled waveform kernels share one argument contract (csrc/wave_tiles.h): a misaligned list, a negative
    count, a count without a list, non-positive sizes, a dense grid beyond INT_MAX and (the fp32 PWG blocks) a NULL operand are
    A3T_EINVAL.  Every row has to be refused before any HIP call: the pointers are host memory."""
    import ctypes
    from a3t_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    x, y, cu, w0, b0, w1, b1, sk, tl = (ctypes.c_void_p(a + 256 * i) for i in range(9))
    f = lib.a3t_pwg_block_f16
    einval = -22                                                                               # A3T_EINVAL
    assert f(x, x, cu, w0, b0, w1, b1, sk, None, 0, 1, 1, 1, None) == einval                    # x_in == x_out
    assert f(x, ctypes.c_void_p(a + 16), cu, w0, b0, w1, b1, sk, None, 0, 1, 4, 1, None) == einval   # overlapping
    assert f(x, y, cu, w0, b0, w1, b1, sk, ctypes.c_void_p(tl.value + 4), 1, 1, 1, 1, None) == einval  # misaligned tile list
    assert f(x, y, ctypes.c_void_p(cu.value + 2), w0, b0, w1, b1, sk, None, 0, 1, 1, 1, None) == einval
    for B, Tw, dil in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert f(x, y, cu, w0, b0, w1, b1, sk, None, 0, B, Tw, dil, None) == einval
    assert f(x, y, cu, w0, b0, w1, b1, sk, tl, -1, 1, 1, 1, None) == einval
    assert lib.a3t_cast_f16_sat(ctypes.c_void_p(x.value + 4), y, 8, None) == einval
    assert lib.a3t_cast_f16_sat(x, y, -1, None) == einval

    pointers = dict(x=x, y=y, cu=cu, wt0=w0, b0=b0, wt1=w1, b1=b1, skips=sk, g=ctypes.c_void_p(a + 256 * 9), R=None, acc=None,
                    stream=None)
    good = dict(pointers, alpha=1.0, acc_add=0, slope=0.1, B=1, Tw=1, dil=1, C=32, taps=3, K=7)
    rows = _refusal_rows(tl.value)
    assert len(rows) == 12 + 28 + 4 + 16 + 1
    for name, change in rows:
        ragged = name == "a3t_pwg_block_ragged"
        v = dict(good, tiles=tl.value if ragged else None, ntiles=1 if ragged else 0)
        assert change and set(change) <= set(ENTRY_ARGS[name]) and any(v[k] != change[k] for k in change)
        v.update(change)
        v["tiles"] = None if v["tiles"] is None else ctypes.c_void_p(v["tiles"])
        assert getattr(lib, name)(*(v[k] for k in ENTRY_ARGS[name])) == einval, (name, change)


def test_constructor_refuses_f16_without_the_fused_v1_plan():
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    cfg, state = R.vocoder_state(seed=4)
    with pytest.raises(ValueError):
        ParallelWaveGANGeneratorHIP(state, device="cpu", compute="f16", fused=False)
    with pytest.raises(ValueError):
        ParallelWaveGANGeneratorHIP(state, device="cpu", compute="f16", residual_channels=32)
    with pytest.raises(ValueError):
        ParallelWaveGANGeneratorHIP(state, device="cpu", compute="f16", aux_channels=40)
    with pytest.raises(ValueError):
        ParallelWaveGANGeneratorHIP(state, device="cpu", compute="bf16")
    gen = ParallelWaveGANGeneratorHIP(state, device="cpu", compute="f16")
    assert gen.compute == "f16" and gen.fused and gen.margin_frames == ParallelWaveGANGeneratorHIP(state, device="cpu").margin_frames
    assert gen.blocks[0]["w0h"].dtype == torch.float16
    assert ParallelWaveGANGeneratorHIP(state, device="cpu").compute == "f32"
