"""The batched duration model on the MI355X: the length-aware row kernels (the RAGGED instantiations in
csrc/norm_reduce.hip and csrc/convmod_attn.hip), the engine's ragged block
forward and FS2DurationModel.forward_ids_batch / predict_frames_batch / duration_fn(...).batch against the reference's own
outputs in tests/golden/fs2_duration.{npz,json} and the CPU restatement tests/fs2_ragged_ref.py."""
import json
import math
import os

import numpy as np
import pytest
import torch

import fs2_ragged_ref as R
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"

_MODELS = {}


def _model(case):
    if case not in _MODELS:
        from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
        cfg, p = R.checkpoint(R.meta(), case)
        _MODELS[case] = FS2DurationModel(FS2DurationConfig.from_espnet(cfg), DEV).load_state_dict(
            {"tts." + k: v for k, v in p.items()})
    return _MODELS[case]


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


# --------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("T,lens", [(7, [1, 2, 7, 5]), (130, [1, 2, 130, 65, 64, 100]), (301, [301, 1, 257, 77]),
                                    (640, [640, 513, 3]), (2100, [2100, 1500])])
def test_ragged_softmax_against_fp64(T, lens):
    """Against the fp64 formula built per row at its own length (rel_shift_legacy on the n x n block); the bounds of
    test_relpos_softmax.  Keys and query rows >= n: exactly 0, whatever the output held."""
    from a3t_amd import ops
    B, H = len(lens), 1 if T > 2048 else 2
    g = torch.Generator().manual_seed(T)
    ac = torch.randn(B, H, T, T, generator=g) * 3.0
    bd = torch.randn(B, H, T, T, generator=g) * 3.0
    scale = 1.0 / math.sqrt(48)
    probs = torch.full((B, H, T, T), float("nan"), device=DEV)
    ops.relpos_softmax_fwd_ragged(ac.to(DEV), bd.to(DEV), _lens(lens), probs, B, H, T, scale)
    torch.cuda.synchronize()
    got = probs.cpu()
    want = R.ragged_softmax(ac.double(), bd.double(), lens, scale)
    for b, n in enumerate(lens):
        assert torch.all(got[b, :, n:, :] == 0) and torch.all(got[b, :, :, n:] == 0), (b, n)
        err = (got[b, :, :n, :n].double() - want[b, :, :n, :n]).abs()
        tol = 1e-6 + 1e-4 * want[b, :, :n, :n].abs()
        print(f"T={T} n={n}: max err {err.max().item():.3g}")
        assert torch.all(err <= tol), (b, n, err.max().item())
        assert (got[b, :, :n, :n].sum(-1) - 1).abs().max() < 1e-5


def test_ragged_softmax_of_a_full_row_is_the_plain_kernel():
    """lens[b] = T: the shift is the plain legacy rel_shift and nothing is masked -- bit for bit a3t_relpos_softmax_fwd."""
    from a3t_amd import ops
    B, H, T = 2, 2, 100
    g = torch.Generator().manual_seed(3)
    ac = (torch.randn(B, H, T, T, generator=g) * 3.0).to(DEV)
    bd = (torch.randn(B, H, T, T, generator=g) * 3.0).to(DEV)
    a, b = torch.empty_like(ac), torch.empty_like(ac)
    ops.relpos_softmax_fwd(ac, bd, torch.ones(B, T, dtype=torch.uint8, device=DEV), a, B, H, T, 0.125)
    ops.relpos_softmax_fwd_ragged(ac, bd, _lens([T, T]), b, B, H, T, 0.125)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_ragged_softmax_of_a_full_long_row_is_the_plain_kernel():
    """The same on the three-pass path of very long rows (T > 2048, NV == 0)."""
    from a3t_amd import ops
    B, H, T = 1, 1, 2100
    g = torch.Generator().manual_seed(4)
    ac = (torch.randn(B, H, T, T, generator=g) * 3.0).to(DEV)
    bd = (torch.randn(B, H, T, T, generator=g) * 3.0).to(DEV)
    a, b = torch.empty_like(ac), torch.empty_like(ac)
    ops.relpos_softmax_fwd(ac, bd, torch.ones(B, T, dtype=torch.uint8, device=DEV), a, B, H, T, 0.125)
    ops.relpos_softmax_fwd_ragged(ac, bd, _lens([T]), b, B, H, T, 0.125)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_ragged_softmax_refuses_bf16():
    from a3t_amd import _lib, ops
    B, H, T = 1, 1, 16
    ac = torch.zeros(B, H, T, T, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.A3TLibraryError):
        ops.relpos_softmax_fwd_ragged(ac, ac, _lens([T]), torch.zeros_like(ac), B, H, T, 1.0)
    f = torch.zeros(B, H, T, T, device=DEV)
    with pytest.raises(_lib.A3TLibraryError):
        ops.relpos_softmax_fwd_ragged(f, f, _lens([T]), torch.zeros_like(ac), B, H, T, 1.0)


@pytest.mark.parametrize("C", [384, 80])
@pytest.mark.parametrize("K", [5, 7, 31])
def test_ragged_glu_dwconv_against_torch(K, C):
    """Per row at its own length against torch (GLU, grouped Conv1d with zero padding); the bounds of test_glu_dwconv."""
    from a3t_amd import ops
    import torch.nn.functional as F
    T, lens = 150, [150, 1, 64, 65, 3, 129]
    B = len(lens)
    g = torch.Generator().manual_seed(K * 1000 + C)
    x = torch.randn(B, T, 2 * C, generator=g)
    w = torch.randn(C, K, generator=g) / K ** 0.5
    bias = torch.randn(C, generator=g)
    glu = torch.full((B * T, C), float("nan"), device=DEV)
    z = torch.full((B * T, C), float("nan"), device=DEV)
    ops.glu_dwconv_fwd_ragged(x.view(B * T, 2 * C).to(DEV), w.to(DEV), bias.to(DEV), glu, z, _lens(lens), B, T)
    torch.cuda.synchronize()
    glu, z = glu.cpu().view(B, T, C), z.cpu().view(B, T, C)
    for b, n in enumerate(lens):
        want_glu = F.glu(x[b, :n].double(), dim=-1)
        want_z = F.conv1d(want_glu.t()[None], w.double()[:, None], bias.double(), padding=(K - 1) // 2, groups=C)[0].t()
        assert torch.all(glu[b, n:] == 0) and torch.all(z[b, n:] == 0), (b, n)
        for got, want in ((glu[b, :n], want_glu), (z[b, :n], want_z)):
            err = (got.double() - want).abs()
            assert torch.all(err <= 2e-5 + 1e-4 * want.abs()), (b, n, err.max().item())


@pytest.mark.parametrize("C", [384, 80])
@pytest.mark.parametrize("K", [5, 7])
def test_ragged_glu_dwconv_at_full_length_is_the_plain_kernel(K, C):
    """lens[b] = T: bit for bit a3t_glu_dwconv_fwd.  T = 70 is one whole 64-row tile and a partial one, C a whole and a
    partial 64-channel block, K the generic tap loop (5) and the register-blocked K == KT path (7)."""
    from a3t_amd import ops
    B, T = 2, 70
    g = torch.Generator().manual_seed(K * 1000 + C + 1)
    x = torch.randn(B * T, 2 * C, generator=g).to(DEV)
    w = (torch.randn(C, K, generator=g) / K ** 0.5).to(DEV)
    bias = torch.randn(C, generator=g).to(DEV)
    glu0, z0 = torch.empty(B * T, C, device=DEV), torch.empty(B * T, C, device=DEV)
    glu1, z1 = torch.full_like(glu0, float("nan")), torch.full_like(z0, float("nan"))
    ops.glu_dwconv_fwd(x, w, bias, glu0, z0, T)
    ops.glu_dwconv_fwd_ragged(x, w, bias, glu1, z1, _lens([T, T]), B, T)
    torch.cuda.synchronize()
    assert torch.equal(glu0, glu1)
    assert torch.equal(z0, z1)


@pytest.mark.parametrize("D", [384, 256, 100, 640])
def test_ragged_layernorm(D):
    """Valid rows against fp64 (atol 2e-5, rtol 1e-5) and bit for bit the plain kernel's; exact zeros behind a length."""
    from a3t_amd import ops
    T, lens = 37, [37, 1, 20, 36]
    B = len(lens)
    g = torch.Generator().manual_seed(D)
    x = torch.randn(B * T, D, generator=g) * 2.0 + 0.5
    gam = 1.0 + 0.2 * torch.rand(D, generator=g)
    bet = 0.1 * torch.randn(D, generator=g)
    xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    y = torch.full((B * T, D), float("nan"), device=DEV)
    mean, rstd = torch.empty(B * T, device=DEV), torch.empty(B * T, device=DEV)
    ops.layernorm_fwd_ragged(xd, gd, bd, y, mean, rstd, _lens(lens), B, T, 1e-12)
    y0 = torch.empty_like(y)
    ops.layernorm_fwd(xd, gd, bd, y0, torch.empty_like(mean), torch.empty_like(rstd), 1e-12)
    y2 = torch.full_like(y, float("nan"))
    ops.layernorm_fwd_ragged(xd, gd, bd, y2, None, None, _lens(lens), B, T, 1e-12)
    torch.cuda.synchronize()
    want = torch.nn.functional.layer_norm(x.double(), (D,), gam.double(), bet.double(), 1e-12).view(B, T, D)
    got, plain = y.cpu().view(B, T, D), y0.cpu().view(B, T, D)
    assert torch.equal(y, y2)
    for b, n in enumerate(lens):
        assert torch.all(got[b, n:] == 0), (b, n)
        err = (got[b, :n].double() - want[b, :n]).abs()
        assert torch.all(err <= 2e-5 + 1e-5 * want[b, :n].abs()), (b, n, err.max().item())
        assert torch.equal(got[b, :n], plain[b, :n])


@pytest.mark.parametrize("D", [384, 256, 100, 640])
def test_ragged_layernorm_does_not_read_behind_a_length(D):
    """x is NaN behind every row's length: exact zeros there, finite valid rows, and the bits that finite padding gives."""
    from a3t_amd import ops
    T, lens = 37, [37, 1, 20, 36]
    B = len(lens)
    g = torch.Generator().manual_seed(D)
    x = torch.randn(B, T, D, generator=g) * 2.0 + 0.5
    gd = (1.0 + 0.2 * torch.rand(D, generator=g)).to(DEV)
    bd = (0.1 * torch.randn(D, generator=g)).to(DEV)
    xn = x.clone()
    for b, n in enumerate(lens):
        xn[b, n:] = float("nan")
    out = []
    for src in (x, xn):
        y = torch.full((B * T, D), float("nan"), device=DEV)
        mean, rstd = torch.full((B * T,), float("nan"), device=DEV), torch.full((B * T,), float("nan"), device=DEV)
        ops.layernorm_fwd_ragged(src.view(B * T, D).to(DEV), gd, bd, y, mean, rstd, _lens(lens), B, T, 1e-12)
        out.append((y.view(B, T, D), mean.view(B, T), rstd.view(B, T)))
    torch.cuda.synchronize()
    for fin, nan in zip(*out):
        assert torch.isfinite(nan).all()
        assert torch.equal(fin, nan)
    y = out[1][0]
    for b, n in enumerate(lens):
        assert torch.all(y[b, n:] == 0), (b, n)
        assert torch.all(out[1][1][b, n:] == 0) and torch.all(out[1][2][b, n:] == 0), (b, n)


# ---------------------------------------------------------------------------------------------------------- the engine
def test_block_forward_against_the_cpu_restatement():
    """Intermediate tensors: the output of every encoder block of a ragged batch against tests/fs2_ragged_ref.py, valid rows
    within 1e-4 of the tensor's scale (the bound test_model_against_reference puts on hs)."""
    m, meta, z = _model("small_c384"), R.meta(), R.arrays()
    cfg, p = R.checkpoint(meta, "small_c384")
    ids, lens = R.fixture_batch(z, meta, "small_c384")
    ids, lens = np.ascontiguousarray(ids[:4, :130]), lens[:4]
    keep = {}
    with torch.no_grad():
        R.ragged_forward(p, cfg["tts_conf"], ids, lens, keep=keep)
    B, T, d = len(lens), 130, m.c.adim
    dl = _lens(lens)
    x = torch.empty(B * T, d, device=DEV)
    from a3t_amd import ops
    ops.embed_finish_fwd(None, m.store.p["temb"], m._seg0, torch.from_numpy(ids).to(DEV), None,
                         torch.zeros(B * T, dtype=torch.int64, device=DEV), x, B, 0, T, d, math.sqrt(d))
    for i in range(m.c.enc_blocks):
        x = m.eng.block_fwd(f"enc.{i}", x, m.eng.pe[:T], None, B, T, lens=dl)
        got = x.cpu().view(B, T, d)
        assert torch.isfinite(got).all()
        for b, n in enumerate(lens):
            ref = keep[f"enc.{i}"][b, :n]
            err = (got[b, :n] - ref).abs().max().item()
            assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (i, b, n, err)


def test_lens_needs_fp32_eval_forward_only():
    from a3t_amd.engine import MLMEngine
    m = _model("small_c384")
    B, T = 2, 8
    x = torch.zeros(B * T, m.c.adim, device=DEV)
    lens = _lens([8, 5])
    for kw in (dict(compute="bf16", training=False), dict(compute="f32", training=True)):
        eng = MLMEngine(m.c, m.store, **kw)
        with pytest.raises(ValueError, match="fp32 compute, eval mode"):
            eng.block_fwd("enc.0", x, eng.pe[:T], None, B, T, lens=lens)
    out = m.eng.block_fwd("enc.0", x, m.eng.pe[:T], None, B, T, lens=lens)      # the duration model's own engine takes it
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------ the whole model
@pytest.mark.parametrize("case", ["lj", "lj_xadd", "lj_xcat", "small_c384"])
def test_forward_ids_batch_against_reference(case):
    """The fixture's five lengths as ONE batch: the bounds of test_model_against_reference (log domain <= 1e-4, frames exact
    away from .5 ties by the 1e-3 rule, which leaves out at most one element per row; |dframes| <= 1; hs at T = 33)."""
    meta, z = R.meta(), R.arrays()
    m = _model(case)
    bias = m.speaker_bias(z[f"{case}.spembs"]) if f"{case}.spembs" in z else None
    ids, lens = R.fixture_batch(z, meta, case)
    hs, logd, frames = m.forward_ids_batch(torch.from_numpy(ids).to(DEV), _lens(lens), bias)
    torch.cuda.synchronize()
    assert hs.shape == (len(lens), max(lens), m.c.adim) and logd.shape == frames.shape == ids.shape
    hs, logd, frames = hs.cpu().numpy(), logd.cpu().numpy(), frames.cpu().numpy()
    assert np.isfinite(logd).all()
    for b, T in enumerate(lens):
        p = f"{case}.T{T}."
        err = np.abs(logd[b, :T] - z[p + "logd"]).max()
        print(f"{case} T={T}: max |dlogd| {err:.3g}")
        assert err <= 1e-4, (T, err)
        far = R.tie_distance(z[p + "expm1"]) > 1e-3
        assert far.sum() >= T - 1
        assert np.array_equal(frames[b, :T][far], z[p + "frames"][far]), T
        assert np.abs(frames[b, :T] - z[p + "frames"]).max() <= 1
        if T == meta["hs_length"]:
            ref = z[p + "hs"]
            e = np.abs(hs[b, :T] - ref).max()
            assert e <= 1e-4 * max(1.0, np.abs(ref).max()), e


@pytest.mark.parametrize("case", ["lj", "lj_xcat"])
def test_padding_cannot_leak(case):
    """The same batch twice: pad ids 0 over a zeroed workspace, then random valid pad ids with every workspace buffer
    pre-filled with NaN.  Same shapes, same kernels: logd and frames of all valid positions are equal bit for bit, and
    finite."""
    meta, z = R.meta(), R.arrays()
    m = _model(case)
    bias = m.speaker_bias(z[f"{case}.spembs"]) if f"{case}.spembs" in z else None
    ids0, lens = R.fixture_batch(z, meta, case)
    ids1, _ = R.fixture_batch(z, meta, case, pad_ids=np.random.RandomState(9))
    assert not np.array_equal(ids0, ids1)
    dl = _lens(lens)
    m.forward_ids_batch(torch.from_numpy(ids0).to(DEV), dl, bias)        # (allocates every buffer of this shape)
    torch.cuda.synchronize()
    runs = []
    for ids, fill in ((ids0, 0.0), (ids1, float("nan"))):
        for t in m.ws.bufs.values():
            if t.is_floating_point():
                t.fill_(fill)
            else:
                t.fill_(0 if fill == 0.0 else 1 << 40)
        _, logd, frames = m.forward_ids_batch(torch.from_numpy(ids).to(DEV), dl, bias)
        torch.cuda.synchronize()
        runs.append((logd.cpu().numpy().copy(), frames.cpu().numpy().copy()))
    for b, n in enumerate(lens):
        assert np.isfinite(runs[1][0][b, :n]).all()
        assert np.array_equal(runs[0][0][b, :n].view(np.int32), runs[1][0][b, :n].view(np.int32)), (b, n)
        assert np.array_equal(runs[0][1][b, :n], runs[1][1][b, :n]), (b, n)


def _lj_records(meta):
    return [r for r in meta["duration_predict"] if r["model"] == "lj" and not r["spembs"]]


def test_batch_matches_duration_predict_bit_for_bit():
    """The 11 recorded `lj` phone lists in ONE call: the seconds the reference's duration_predict gave, bit for bit."""
    meta = R.meta()
    recs = _lj_records(meta)
    assert len(recs) == 11
    fn = _model("lj").duration_fn(meta["fs"], meta["hop"])
    got = fn.batch([r["phns"] for r in recs])
    assert len(got) == len(recs)
    for g, r in zip(got, recs):
        assert all(type(v) is float for v in g)
        assert g == r["seconds"], (r["phns"], g, r["seconds"])


def test_batch_with_speaker_matches_duration_predict():
    meta, z = R.meta(), R.arrays()
    rec = [r for r in meta["duration_predict"] if r["spembs"]][0]
    fn = _model(rec["model"]).duration_fn(meta["fs"], meta["hop"], spembs=z[f"{rec['model']}.spembs"])
    other = ["sp", "K", "AE1", "T", "sp", "D", "AO1", "G"]
    got = fn.batch([other, rec["phns"]])
    assert got[1] == rec["seconds"] and got[0] == fn(other)


def test_chunking_does_not_change_the_result():
    meta = R.meta()
    m = _model("lj")
    lists = [r["phns"] for r in _lj_records(meta)]
    fn = m.duration_fn(meta["fs"], meta["hop"])
    want = fn.batch(lists)
    lengths = [len(x) + 1 for x in lists]
    cap = 4 * m.c.heads * max(lengths) ** 2
    chunks = m._chunks(lengths, cap)
    assert len(chunks) >= 2 and any(len(c) > 1 for c in chunks)
    assert fn.batch(lists, max_score_elems=cap) == want
    assert fn.batch(lists, max_score_elems=1) == want           # every list alone: the B = 1 path
    assert [fn(x) for x in lists] == want
    # order and duplicates are the caller's
    assert fn.batch(lists[::-1] + lists[:2]) == want[::-1] + want[:2]


def test_batch_of_one_list_is_predict_frames():
    m = _model("lj")
    phns = ["sp", "HH", "AH0", "L", "OW1", "sp", "W", "ER1", "L", "D"]
    a = m.predict_frames(phns)
    b = m.predict_frames_batch([phns])
    assert len(b) == 1 and b[0].dtype == np.int64 and np.array_equal(a, b[0])
    assert m.predict_frames_batch([]) == []


def test_batch_copies_to_the_host_once_per_call():
    meta = R.meta()
    m = _model("lj")
    lists = [r["phns"] for r in _lj_records(meta)]
    fn = m.duration_fn(meta["fs"], meta["hop"])
    fn.batch(lists)
    cap = 4 * m.c.heads * max(len(x) + 1 for x in lists) ** 2
    n = {"sync": 0}
    orig = torch.Tensor.cpu

    def counting(self, *a, **k):
        n["sync"] += 1
        return orig(self, *a, **k)
    torch.Tensor.cpu = counting
    try:
        out = fn.batch(lists)
        one = n["sync"]
        fn.batch(lists, max_score_elems=cap)       # several chunks: still one copy down
    finally:
        torch.Tensor.cpu = orig
    assert one == 1 and n["sync"] == 2 and len(out) == len(lists)


def test_edit_batch_with_native_durations():
    """SpeechEditor.edit_batch with the native model (whose duration_fn has .batch): the four sedit.json edit kinds in ONE batch
    plan exactly as the oracle's restatement of prepare_features_with_duration does when it is driven by the reference's
    recorded duration_predict outputs -- what test_speech_editor_with_native_durations checks for single edits."""
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    from a3t_amd.sedit import EditRequest, SpeechEditor
    from a3t_amd.task import MLMTask
    from test_gpu_e2e import _task_args
    meta = R.meta()
    rec = {tuple(r["phns"]): r["seconds"] for r in _lj_records(meta)}
    fx = json.load(open(os.path.join(G, "sedit.json")))
    oc = O.tiny_config()
    wavs = np.load(os.path.join(G, "sedit_wav.npz"))
    reqs, want = [], []
    for kind in ("replace", "mask", "append", "delete"):
        case = [c for c in fx["cases"] if c["kind"] == kind][0]
        wav = (0.1 * np.random.RandomState(5).standard_normal(wavs[case["wav"] + ".in"].shape[0])).astype(np.float32)
        args = (case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"], case["old_str"], case["new_str"])
        ms, me, op, nph, rep, add = O.sedit_phone_spans(*args)
        want.append(O.sedit_plan_edit(wav, oc.fs, oc.hop_length, ms, me, op, nph, rep, add, lambda ph: list(rec[tuple(ph)]),
                                      case["new_str"], **case["opts"]))
        reqs.append(EditRequest(wav, *args, **case["opts"]))
    native = _model("lj").duration_fn(oc.fs, oc.hop_length)
    calls = {"batch": 0, "plain": 0}

    def counted(phns):
        calls["plain"] += 1
        return native(phns)

    def counted_batch(lists):
        calls["batch"] += 1
        return native.batch(lists)
    counted.batch = counted_batch
    model = MLMTask.build_model(_task_args(oc), device=DEV)
    state = O.procedural_state(O.param_shapes(oc), 1)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    fe = LogMelFbank(fs=oc.fs, n_fft=oc.n_fft, win_length=oc.win_length, hop_length=oc.hop_length, n_mels=oc.n_mels,
                     fmin=oc.fmin, fmax=oc.fmax, device=DEV)
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob, mean_phn_span=oc.mean_phn_span,
                        sega_emb=True)
    ids = lambda phns: np.array([2 + sum(map(ord, ph)) % (oc.vocab - 4) for ph in phns], dtype=np.int64)
    ed = SpeechEditor(model, coll, None, ids, counted)
    res = ed.edit_batch(reqs)
    assert calls == {"batch": 1, "plain": 0}
    assert len(res) == 4
    for r, w in zip(res, want):
        assert tuple(r["old_span_boundary"]) == tuple(w[4]) and tuple(r["new_span_boundary"]) == tuple(w[5])
        assert r["feat"].shape[1] == 80 and torch.isfinite(torch.as_tensor(r["feat"])).all()
    from a3t_amd import sedit
    plans, _ = sedit.plan_batch(reqs, oc.fs, oc.hop_length, native, ids)
    for p, w in zip(plans, want):
        assert np.array_equal(p.wav, w[0])
        assert list(p.phns) == list(w[1]) and list(p.align_start) == list(w[2]) and list(p.align_end) == list(w[3])
        assert tuple(p.old_span_boundary) == tuple(w[4]) and tuple(p.new_span_boundary) == tuple(w[5])
