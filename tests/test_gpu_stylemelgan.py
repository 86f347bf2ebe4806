"""StyleMelGAN generator on the device (a3t_amd/vocoder.py::StyleMelGANGeneratorHIP, csrc/stylemelgan.hip): the two kernels against
fp64 torch, every TADEResBlock alone against the restatement's block, the whole generator against the reference's outputs
(tests/golden/stylemelgan.{npz,json}), ragged batches and SpeechEditor with this vocoder.

Tolerance of every numeric comparison (the rule of test_gpu_melgan.py::_check): the yardstick is the fp64 result, the bound 4 x F
(stylemelgan_ref.bound), where F is what an fp32 evaluation by the reference (fixture cases) or by torch on the CPU (kernel and
block cases, computed here) loses against fp64 on the same input, floored at 1e-6 of scale.  The block tests hold the kernels; the
plan as a whole amplifies rounding.  Measured device values: profiles/stylemelgan_parity.txt."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stylemelgan_ref as R
from test_gpu_melgan import _check, _tiles

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
B, T = 2, 300      # one full tile and a partial one
SENTINEL = 7.5
PLAIN, TADE, GATE = 0, 1, 2


def _rows(n, u):
    return -(-n // u)


# ----------------------------------------------------------------------------------------------------------- a3t_smg_conv
# (mode, Cin, taps, dil, up, ux, ur, gate, bias, logit scale)
CONV_CASES = [
    (PLAIN, 80, 9, 1, 1, 1, 1, None, True, 1), (PLAIN, 64, 9, 2, 5, 1, 1, None, True, 1), (PLAIN, 16, 5, 3, 3, 1, 1, None, False, 1),
    (PLAIN, 64, 9, 1, 2, 1, 1, None, True, 1),
    (TADE, 64, 9, 1, 1, 1, 1, None, True, 1), (TADE, 64, 9, 2, 1, 2, 1, None, True, 1), (TADE, 64, 5, 3, 1, 3, 1, None, False, 1),
    (TADE, 64, 9, 1, 1, 5, 1, None, True, 1), (TADE, 64, 9, 1, 2, 2, 1, None, True, 1),
    (GATE, 64, 9, 1, 1, 1, 1, "softmax", True, 1), (GATE, 64, 9, 2, 1, 1, 2, "softmax", True, 1),
    (GATE, 64, 9, 2, 1, 1, 3, "sigmoid", True, 1), (GATE, 64, 9, 2, 1, 1, 5, "softmax", False, 1),
    (GATE, 64, 5, 3, 1, 1, 0, "sigmoid", True, 1), (GATE, 64, 9, 2, 1, 1, 0, "softmax", True, 30), (GATE, 64, 9, 1, 3, 1, 1, "sigmoid", True, 1),
]


@functools.lru_cache(maxsize=None)
def _conv_case(case):
    """Inputs and the CPU references of one convolution, computed once: both rows at full length, and row 1 cut to 257 and 5
    samples run alone, in fp64 and fp32."""
    mode, Cin, taps, dil, up, ux, ur, gate, bias, ls = case
    N = 64 if mode == PLAIN else 128
    g = torch.Generator().manual_seed(500 + CONV_CASES.index(case))
    x = torch.randn(B, _rows(T, up), Cin, generator=g)
    m = torch.randn(B, _rows(T, ux), 64, generator=g) * 0.5 + 1.0
    Rr = torch.randn(B, _rows(T, ur), 64, generator=g) if ur else None
    w = torch.randn(N, Cin, taps, generator=g) / (Cin * taps) ** 0.5
    w[:64] *= ls
    bv = torch.randn(N, generator=g) * 0.3 if bias else None
    st = torch.stack([torch.randn(B, 64, generator=g) * 0.2 + 1.0, torch.rand(B, 64, generator=g) + 0.5], dim=1)      # mean | rstd

    def run(b, n, dt):      # row b cut to n samples, alone -> [n][64]
        xu = x[b].to(dt).repeat_interleave(up, dim=0)[:n].t()[None]
        v = F.conv1d(xu, w.to(dt), None if bv is None else bv.to(dt), padding=(taps - 1) // 2 * dil, dilation=dil)[0].t()
        if mode == PLAIN:
            return v
        if mode == TADE:
            mu = m[b].to(dt).repeat_interleave(ux, dim=0)[:n]
            return v[:, :64] * ((mu - st[b, 0].to(dt)) * st[b, 1].to(dt)) + v[:, 64:]
        ga = torch.softmax(v[:, :64], dim=1) if gate == "softmax" else torch.sigmoid(v[:, :64])
        y = ga * torch.tanh(v[:, 64:])
        return y + Rr[b].to(dt).repeat_interleave(ur, dim=0)[:n] if ur else y

    ref = {}
    for dt in (torch.float64, torch.float32):
        ref[dt] = {n: run(1, n, dt) for n in (257, 5)}
        ref[dt][T] = torch.stack([run(b, T, dt) for b in range(B)])
    return x, m, Rr, w, bv, st, ref


def _launch(case, ten, Bn, Tw, tiles=None):
    """The kernel over x / m / R given as [Bn][rows][C] CPU tensors -> y [Bn][Tw][64] on the device, sentinel-filled first."""
    from a3t_amd import ops
    from a3t_amd.vocoder import pack_hifigan_conv
    mode, Cin, taps, dil, up, ux, ur, gate, bias, ls = case
    x, m, Rr, w, bv, st = ten
    d = lambda t: None if t is None else t.contiguous().to(DEV)      # noqa: E731
    y = torch.full((Bn * Tw, 64), SENTINEL, device=DEV)
    xd = d(x).view(-1, Cin)
    keep = xd.clone()
    ops.smg_conv(xd, d(pack_hifigan_conv(w)), d(bv), y, Bn, Tw, dil=dil, up=up, mode=mode, m=d(m).view(-1, 64) if mode == TADE else None,
                 stats=d(st) if mode == TADE else None, ux=ux, R=d(Rr).view(-1, 64) if (mode == GATE and ur) else None, ur=max(ur, 1),
                 sigmoid=gate == "sigmoid", tiles=tiles)
    assert torch.equal(torch.isnan(xd), torch.isnan(keep)) and torch.equal(xd.nan_to_num(), keep.nan_to_num())      # input untouched
    return y.view(Bn, Tw, 64)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_smg_conv(case):
    """Dense; ragged with row 1 ending one sample into a tile (257) and inside the halo (5), NaN in every padding row: nothing
    behind W_b is written and a ragged row is the row run alone bit for bit."""
    mode, Cin, taps, dil, up, ux, ur, gate, bias, ls = case
    x, m, Rr, w, bv, st, ref = _conv_case(case)
    scale = float(ref[torch.float64][T].abs().max())
    tag = "smg_conv " + "-".join(str(v) for v in case)
    dense = _launch(case, (x, m, Rr, w, bv, st), B, T)
    _check(f"{tag} dense", dense, ref[torch.float64][T], ref[torch.float32][T], scale)
    for W1 in (257, 5):
        def cut(t, u):      # row 1 valid for ceil(W1 / u) rows, NaN behind
            if t is None:
                return None
            t = t.clone()
            t[1, _rows(W1, u):] = float("nan")
            return t
        y = _launch(case, (cut(x, up), cut(m, ux), cut(Rr, max(ur, 1)), w, bv, st), B, T, tiles=_tiles([T, W1]))
        assert torch.equal(y[0], dense[0]), tag                                  # the full row: the dense run's bits
        _check(f"{tag} ragged ({T}, {W1})", y[1, :W1], ref[torch.float64][W1], ref[torch.float32][W1], scale)
        assert bool((y[1, W1:] == SENTINEL).all()), tag                           # nothing behind W_b is written
        one = lambda t, u: None if t is None else t[1:2, :_rows(W1, u)]          # noqa: E731
        alone = _launch(case, (one(x, up), one(m, ux), one(Rr, max(ur, 1)), w, bv, st[1:2]), 1, W1)
        assert torch.equal(y[1, :W1], alone[0]), (tag, W1, float((y[1, :W1] - alone[0]).abs().max()))


def test_smg_conv_refuses_what_it_was_not_built_for():
    from a3t_amd import ops
    from a3t_amd._lib import A3TLibraryError
    x, y = torch.zeros(512, 64, device=DEV), torch.zeros(512, 64, device=DEV)
    w = torch.zeros(9 * 64, 64, device=DEV)
    with pytest.raises(ValueError, match="overlaps"):
        ops.smg_conv(x, w, None, x, 1, 512)
    with pytest.raises(ValueError, match="wt must be"):
        ops.smg_conv(x, w, None, y, 1, 512, mode=ops.SMG_GATE)                                   # 64 columns for a 128-column mode
    with pytest.raises(ValueError, match="TADE"):
        ops.smg_conv(x, torch.zeros(9 * 64, 128, device=DEV), None, y, 1, 512, mode=ops.SMG_TADE)
    with pytest.raises(A3TLibraryError):
        ops.smg_conv(x, torch.zeros(11 * 64, 64, device=DEV), None, y, 1, 512)                   # 11 taps
    with pytest.raises(A3TLibraryError):
        ops.smg_conv(x, w, None, y, 1, 512, dil=0)
    x8 = torch.zeros(512, 8, device=DEV)
    with pytest.raises(A3TLibraryError):
        ops.smg_conv(x8, torch.zeros(9 * 8, 64, device=DEV), None, y, 1, 512)                    # Cin 8
    assert bool((y == 0).all())      # nothing was launched


# ---------------------------------------------------------------------------------------------------------- a3t_smg_stats
@functools.lru_cache(maxsize=None)
def _stats_rows():
    g = torch.Generator().manual_seed(77)
    return {1: torch.randn(1, 64, generator=g), 257: torch.randn(257, 64, generator=g) * 0.7 + 0.2,
            5000: torch.randn(5000, 64, generator=g) * 0.05 + 3.0}      # (mean 3, std 0.05: a sum of squares would lose the variance)


def _stats_ref(x, dt):
    x = x.to(dt)
    return torch.stack([x.mean(0), 1.0 / torch.sqrt(x.var(0, unbiased=False) + 1e-5)])


def test_smg_stats():
    """Mean and rstd of rows of 1 (variance 0), 257 and 5000 samples against fp64, each alone, as row 0 and as row 2 of a ragged
    batch with NaN in the padding: the same bits in every position."""
    from a3t_amd import ops
    rows = _stats_rows()

    def run(xs, lengths=None):
        Bn, Tw = len(xs), max(x.shape[0] for x in xs)
        buf = torch.full((Bn, Tw, 64), float("nan"))
        for b, x in enumerate(xs):
            buf[b, :x.shape[0]] = x
        st = torch.full((Bn, 2, 64), SENTINEL, device=DEV)
        ops.smg_stats(buf.to(DEV).view(-1, 64), st, Bn, Tw, tiles=None if lengths is None else _tiles(lengths))
        return st

    alone = {n: run([x])[0] for n, x in rows.items()}
    for n, x in rows.items():
        r64, r32 = _stats_ref(x, torch.float64), _stats_ref(x, torch.float32)
        _check(f"smg_stats mean, {n} samples", alone[n][0], r64[0], r32[0])
        _check(f"smg_stats rstd, {n} samples", alone[n][1], r64[1], r32[1])
    for order in ((5000, 1, 257), (257, 5000, 1), (1, 257, 5000)):
        st = run([rows[n] for n in order], lengths=list(order))
        for b, n in enumerate(order):
            assert torch.equal(st[b], alone[n]), (order, b, float((st[b] - alone[n]).abs().max()))


def test_smg_stats_of_an_empty_row_and_refusals():
    from a3t_amd import ops
    x = torch.randn(2 * 300, 64, device=DEV)
    st = torch.full((2, 2, 64), SENTINEL, device=DEV)
    ops.smg_stats(x, st, 2, 300, tiles=_tiles([300, 0]))
    assert bool((st[1] == 0).all()) and bool(torch.isfinite(st[0]).all())
    with pytest.raises(ValueError):
        ops.smg_stats(torch.zeros(300, 32, device=DEV), st, 2, 150)
    with pytest.raises(ValueError, match="part"):
        ops.smg_stats(x, st, 2, 300, part=torch.zeros(128, device=DEV))


# --------------------------------------------------------------------------------------------------------------- generator
@functools.lru_cache(maxsize=None)
def _state(name):
    return R.case_state(name)


@functools.lru_cache(maxsize=None)
def _gen(name):
    from a3t_amd.vocoder import StyleMelGANGeneratorHIP
    return StyleMelGANGeneratorHIP(_state(name), device=DEV, **R.CASES[name]["cfg"])


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(G, "stylemelgan.npz")), json.load(open(os.path.join(G, "stylemelgan.json")))


def _inputs(name, Tf, dseed=0):
    case = R.CASES[name]
    return (torch.from_numpy(R.mel_input(Tf, case["seed"], case["cfg"]["aux_channels"])),
            torch.from_numpy(R.noise_input(case["cfg"], Tf, case["seed"] + dseed)))


@functools.lru_cache(maxsize=None)
def _block_refs(name):
    """The restatement's block tensors at the case's longest input, fp64: [(x_in, c_in, x_out, c_out)] per block."""
    case = R.CASES[name]
    blocks = []
    R.generator(_state(name), case["cfg"], *_inputs(name, max(case["frames"])), dtype=torch.float64, blocks=blocks)
    return blocks


@pytest.mark.parametrize("name,k", [("small_sigmoid", k) for k in range(3)] + [("odd", k) for k in range(3)] + [("v1_wn", k) for k in (0, 4, 8)])
def test_tade_res_block_alone(name, k):
    """Block k on the restatement's fp64 block inputs rounded to fp32, against its fp64 block output (x and c); F from torch's fp32
    run of the same block on the same rounded inputs."""
    gen, cfg = _gen(name), R.CASES[name]["cfg"]
    xi, ci, xo, co = _block_refs(name)[k]
    x32, c32 = xi.float(), ci.float()
    rate = int(np.prod(cfg["upsample_scales"][:k]))
    Te = xi.shape[0] // rate
    assert Te * rate == xi.shape[0] and Te == R.n_eff(cfg, max(R.CASES[name]["frames"]))
    ref = {}
    for dt in (torch.float64, torch.float32):
        yx, yc = R.block(R.folded(_state(name), dt), cfg, k, x32.to(dt).t()[None], c32.to(dt).t()[None])
        ref[dt] = (yx[0].t(), yc[0].t())
    # the fp64 block on the rounded inputs is the yardstick; it is the restatement's own output up to that rounding
    assert float((ref[torch.float64][0] - xo).abs().max()) <= 1e-4 * max(1.0, float(xo.abs().max()))
    gx, gc, _ = gen._block(gen.blocks[k], x32.to(DEV).contiguous(), c32.to(DEV).contiguous(), 1, Te, rate, {})
    _check(f"block {name}.{k} x", gx, ref[torch.float64][0], ref[torch.float32][0])
    _check(f"block {name}.{k} c", gc, ref[torch.float64][1], ref[torch.float32][1])


@pytest.mark.parametrize("name", list(R.CASES))
def test_generator_against_the_reference(name):
    arrays, meta = _golden()
    gen, case, info = _gen(name), R.CASES[name], meta["cases"][name]
    assert gen.hop == info["hop"] and gen.noise_upsample_factor == info["noise_factor"]
    assert gen.margin_frames is None and gen.min_frames == 1
    for Tf in case["frames"]:
        want = arrays[f"{name}.T{Tf}.wav64"]
        mel, z = _inputs(name, Tf)
        assert gen.noise_shape(Tf) == tuple(z.shape)
        got = gen.inference(mel, z).cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        err, bound = float(np.abs(got - want).max()), R.bound(info["F"][str(Tf)], R.scale_of(want))
        print(f"generator {name} T={Tf}: device error {err:.3e}, F {info['F'][str(Tf)]:.3e}, bound {bound:.3e}")
        assert err <= bound


def _ragged(name, lengths):
    """(c with NaN padding, z with NaN padding, the per-row inputs) of a batch of rows of `lengths` frames."""
    cfg = R.CASES[name]["cfg"]
    Tm = max(lengths)
    c = torch.full((len(lengths), Tm, cfg["aux_channels"]), float("nan"))
    z = torch.full((len(lengths), R.noise_steps(cfg, Tm), cfg["in_channels"]), float("nan"))
    rows = []
    for b, n in enumerate(lengths):
        mel, zb = _inputs(name, n, dseed=b)
        c[b, :n], z[b, :zb.shape[0]] = mel, zb
        rows.append((mel, zb))
    return c, z, rows


@pytest.mark.parametrize("name,lengths", [("v1_wn", (81, 1, 40)), ("small_sigmoid", (45, 1, 4, 5, 0)), ("odd", (3, 50, 2, 0))])
def test_ragged_batch_equals_the_single_runs(name, lengths):
    """NaN in the padding of c and z: every row is its single run bit for bit and zero behind its end; the caller's tensors are
    untouched."""
    gen = _gen(name)
    c, z, rows = _ragged(name, lengths)
    cd, zd = c.to(DEV), z.to(DEV)
    y = gen.inference(cd, zd, lengths=lengths)
    assert y.shape == (len(lengths), max(lengths) * gen.hop, 1)
    assert torch.equal(cd.cpu().nan_to_num(1e9), c.nan_to_num(1e9)) and torch.equal(zd.cpu().nan_to_num(1e9), z.nan_to_num(1e9))
    for b, n in enumerate(lengths):
        if n:
            alone = gen.inference(*rows[b])
            assert torch.equal(y[b, :n * gen.hop], alone), (b, float((y[b, :n * gen.hop] - alone).abs().max()))
        assert bool((y[b, n * gen.hop:] == 0).all())


def test_dense_batch_equals_ragged_with_equal_lengths_and_random_noise():
    gen = _gen("odd")
    c = torch.stack([_inputs("odd", 50)[0], _inputs("odd", 50)[0].flip(0)])
    z = torch.stack([_inputs("odd", 50)[1], _inputs("odd", 50, 1)[1]])
    dense, rag = gen.inference(c, z), gen.inference(c, z, lengths=(50, 50))
    assert torch.equal(dense, rag)
    assert torch.equal(dense[1], gen.inference(c[1], z[1]))
    y = gen.inference(c[0])      # z=None: torch.randn on the device
    assert y.shape == (50 * gen.hop, 1) and bool(torch.isfinite(y).all()) and not torch.equal(y, dense[0])
    with pytest.raises(ValueError, match=r"expected \(9, 32\)"):
        gen.inference(c[0], z[0, :8])
    with pytest.raises(ValueError, match=r"expected \(2, 9, 32\)"):
        gen.inference(c, z[0])


# --------------------------------------------------------------------------------------------------------- SpeechEditor
class _Vocoder:
    """The generator with reproducible noise: called as a plain callable (what `edit` does) it draws the noise of a T-frame
    utterance from RandomState(9); `inference` passes through."""

    def __init__(self, voc):
        self.voc, self.margin_frames, self.min_frames, self.noise_shape = voc, voc.margin_frames, voc.min_frames, voc.noise_shape

    def noise(self, Tf):
        return np.random.RandomState(9).standard_normal(self.voc.noise_shape(Tf)).astype(np.float32)

    def __call__(self, feat):
        return self.voc.inference(feat, torch.from_numpy(self.noise(feat.shape[0])))

    def inference(self, c, z=None, normalize_before=False, lengths=None):
        return self.voc.inference(c, z, normalize_before, lengths=lengths)


@functools.lru_cache(maxsize=None)
def _editor():
    import test_gpu_sedit_batch as SB
    ed, oc, *_ = SB._editor()      # a fresh editor of our own (that helper is not cached): replacing its vocoder touches no other test
    assert oc.hop_length == 300
    ed.vocoder = _Vocoder(_gen("v1_wn"))
    return ed, SB


def test_speech_editor_batch_of_one_equals_edit():
    ed, SB = _editor()
    r = SB._requests()[0]
    one = ed.edit(*SB._args(r), **SB._opts(r))
    Tf = one["feat"].shape[0]
    got = ed.edit_batch([r], z=[ed.vocoder.noise(Tf)])[0]
    assert got["new_span_boundary"] == one["new_span_boundary"] and torch.equal(got["feat"], one["feat"])
    for k in ("origin", "prediction", "orgin_replaced"):
        assert np.array_equal(got[k], one[k]), (k, float(np.abs(got[k] - one[k]).max()))
    assert np.isfinite(got["prediction"]).all() and float(np.abs(got["prediction"]).max()) > 1e-3
    with pytest.raises(ValueError, match="noise_shape"):
        ed.edit_batch([r], z=[np.zeros(Tf * 300, dtype=np.float32)])


def test_speech_editor_span_only_is_the_splice_from_full_vocoding():
    ed, SB = _editor()
    reqs = SB._requests()[:2]
    flen = [f.shape[0] for _, f, _, _ in ed.decode_batch(reqs)]
    z = [ed.vocoder.noise(n) for n in flen]
    full = ed.edit_batch(reqs, z=z)
    span = ed.edit_batch(reqs, outputs=("orgin_replaced",), z=z)
    for f, s in zip(full, span):
        assert "prediction" not in s and "prediction" in f
        assert np.array_equal(f["orgin_replaced"], s["orgin_replaced"])
