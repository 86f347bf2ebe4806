"""One x-vector per request of a batch on the MI355X: FS2DurationModel.speaker_bias_table / forward_ids_batch(spk_rows=) /
predict_frames_batch(spk_rows=) / duration_fn(...).batch(speakers=), FS2TTSModel.synthesize_batch(speakers=) and
SpeechEditor.edit_batch with EditRequest.spembs, against the reference's own outputs in tests/golden/fs2_speakers.{npz,json}.
Bounds are those of the existing tests: durations and frame counts exact, log-domain durations within 1e-4
(tests/test_gpu_duration*.py), pitch / energy / before / feat_gen / feat_gen_denorm within max(4 F, 1e-4) of scale, F the
reference's own fp32-vs-fp64 distance of the stage (tests/test_gpu_fs2_tts.py)."""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

import fs2_speakers_ref as SR
import fs2_tts_ref as R
import gst_ref as GR
from test_gpu_fs2_tts import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
ROWS = ((0, 2), (1, 7), (2, 33), (0, 7))      # (x-vector, tokens) of the four lists of a batch: ragged, one speaker twice
SWAPPED = ((0, 2), (0, 7), (2, 33), (1, 7))   # the x-vectors of rows 1 and 3 exchanged


@functools.lru_cache(maxsize=None)
def _fixture():
    return R.meta(), SR.meta(), SR.arrays()


@functools.lru_cache(maxsize=None)
def _inputs(case):
    tm, sm, _ = _fixture()
    return SR.inputs(tm, sm, case)


def _lists(case, rows=ROWS):
    tm = _fixture()[0]
    ids, spk, prompt, _, _ = _inputs(case)
    return [SR.phones(tm, ids[T]) for _, T in rows], [spk[k] for k, _ in rows], prompt


def _style(m, prompt):
    return None if prompt is None else m.style_from_prompts(prompt_mels=[prompt])


def _host(out):
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _check_row(case, t, out):
    """One synthesis result (numpy arrays) against fixture run t."""
    tm, sm, z = _fixture()
    run = sm["cases"][case]["runs"][t]
    assert np.array_equal(out["duration"], z[t + ".duration"]), t
    assert out["feat_gen"].shape[0] == run["frames"], t
    assert ("feat_gen_denorm" in out) == tm["cases"][case]["normalize"]
    for k in SR.MEL_STAGES:
        if f"{t}.{k}" not in z:
            continue
        want, F = z[f"{t}.{k}"], run["fp64"][k]
        assert out[k].shape == want.shape and np.isfinite(out[k]).all(), (t, k)
        err = float(np.abs(out[k] - want).max()) / R.scale_of(want)
        print(f"{t} {k}: device error {err:.2e} of scale, F {F:.2e}, bound {SR.mel_bound(F):.2e}")
        assert err <= SR.mel_bound(F), (t, k, err, F)


def _check_logd(case, t, logd):
    z = _fixture()[2]
    err = float(np.abs(logd - z[t + ".logd"]).max())
    print(f"{t} logd: max |dlogd| {err:.3g}")
    assert np.isfinite(logd).all() and err <= SR.LOGD_BOUND, (t, err)


def _synth(m, lists, prompt, **kw):
    out = m.synthesize_batch(lists, prompt_mels=prompt, **kw)
    torch.cuda.synchronize()
    return [_host(o) for o in out]


def _padded(case, rows, pad=None):
    """(ids int64 [B][Tmax], lens) of the rows' token ids; pad: a RandomState that draws valid ids behind every row."""
    tm = _fixture()[0]
    ids = _inputs(case)[0]
    lens = [T for _, T in rows]
    out = np.zeros((len(rows), max(lens)), np.int64) if pad is None else \
        pad.randint(0, len(tm["token_list"]), size=(len(rows), max(lens))).astype(np.int64)
    for b, (_, T) in enumerate(rows):
        out[b, :T] = ids[T]
    return out, lens


# ------------------------------------------------------------------------------------- 1. single calls against the fixture
@functools.lru_cache(maxsize=None)
def _singles(case):
    """Every (x-vector, length) of a model as a single call, computed once: {(k, T): (frames, logd, synthesis result)}."""
    tm = _fixture()[0]
    m = _model(case)
    ids, spk, prompt, _, _ = _inputs(case)
    style = _style(m, prompt)
    got = {}
    for k in range(SR.N_SPEAKERS):
        for T in SR.LENGTHS:
            phns = SR.phones(tm, ids[T])
            bias = m.speaker_bias(spk[k])
            frames = m.predict_frames(phns, bias, style)
            _, logd, _ = m.forward_ids(torch.from_numpy(ids[T]).to(DEV), bias, style)
            logd = logd.cpu().numpy().copy()
            out = m.synthesize(phns, spembs=spk[k], prompt_mel=prompt)
            torch.cuda.synchronize()
            got[(k, T)] = (frames, logd, _host(out))
    return got


@pytest.mark.parametrize("case", SR.MODELS)
def test_single_calls_against_the_reference(case):
    """The unchanged single path for three speakers per model: predict_frames(…, speaker_bias(x)) and synthesize(…, spembs=x)."""
    z = _fixture()[2]
    for (k, T), (frames, logd, out) in _singles(case).items():
        t = SR.tag(case, k, T)
        assert np.array_equal(frames, z[t + ".duration"]), t
        _check_logd(case, t, logd)
        _check_row(case, t, out)


# ----------------------------------------------------------------------------------------- 2. per-row speakers in ONE call
@pytest.mark.parametrize("case", SR.MODELS)
def test_one_call_with_a_speaker_per_row_against_the_reference(case):
    tm, _, z = _fixture()
    m = _model(case)
    lists, xs, prompt = _lists(case)
    assert xs[0] is xs[3] and len({id(x) for x in xs}) == 3
    style = _style(m, prompt)
    table, rows = m.speaker_bias_table(xs)
    assert rows == [0, 1, 2, 0] and table.shape == (3, m.c.adim)
    for r, k in ((0, 0), (1, 1), (2, 2)):          # a table row is the bias of that x-vector alone, bit for bit
        assert torch.equal(table[r:r + 1], m.speaker_bias(_inputs(case)[1][k]))
    # the forward itself: log-domain durations and frames of every row
    ids, lens = _padded(case, ROWS)
    _, logd, frames = m.forward_ids_batch(torch.from_numpy(ids).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV),
                                          table, style, None, torch.tensor(rows, dtype=torch.int32, device=DEV))
    logd, frames = logd.cpu().numpy(), frames.cpu().numpy()
    for b, (k, T) in enumerate(ROWS):
        t = SR.tag(case, k, T)
        _check_logd(case, t, logd[b, :T])
        assert np.array_equal(frames[b, :T], z[t + ".duration"]), t
    # the durations through the public calls
    got = m.predict_frames_batch(lists, table, style=style, spk_rows=rows)
    for b, (k, T) in enumerate(ROWS):
        assert np.array_equal(got[b], z[SR.tag(case, k, T) + ".duration"]) and np.array_equal(got[b], _singles(case)[(k, T)][0])
    if not m.c.use_gst:     # (a GST model's duration_fn takes a waveform and feeds its RAW log-mel: the fixture's is normalised)
        fn = m.duration_fn(tm["fs"], tm["hop"])
        secs = fn.batch(lists, speakers=xs)
        for b, (k, T) in enumerate(ROWS):
            want = ((z[SR.tag(case, k, T) + ".duration"] * tm["hop"]).astype(np.float32) / np.float32(tm["fs"]))[:-1].tolist()
            assert secs[b] == want, (b, secs[b], want)
    # the synthesis
    outs = _synth(m, lists, prompt, speakers=xs)
    for b, (k, T) in enumerate(ROWS):
        _check_row(case, SR.tag(case, k, T), outs[b])
        assert np.array_equal(outs[b]["duration"], _singles(case)[(k, T)][2]["duration"])
        assert outs[b]["feat_gen"].shape == _singles(case)[(k, T)][2]["feat_gen"].shape


# ------------------------------------------------------------------------------------------------ 3. the speaker decides
@pytest.mark.parametrize("case", SR.MODELS)
def test_swapping_two_speakers_changes_exactly_those_rows(case):
    """The x-vectors of rows 1 and 3 (the same 7 tokens) exchanged: those rows now are the other fixture runs, and differ from
    before in their durations or by more than 100 x the bound in the mel; rows 0 and 2 do not change a bit."""
    tm, sm, _ = _fixture()
    m = _model(case)
    lists, xs, prompt = _lists(case)
    lists2, xs2, _ = _lists(case, SWAPPED)
    assert lists2 == lists and xs2[1] is xs[3] and xs2[3] is xs[1]
    a, b = _synth(m, lists, prompt, speakers=xs), _synth(m, lists, prompt, speakers=xs2)
    for r in (0, 2):
        assert set(a[r]) == set(b[r])
        for k in a[r]:
            assert np.array_equal(a[r][k], b[r][k]), (r, k)
    for r in (1, 3):
        t = SR.tag(case, *SWAPPED[r])
        _check_row(case, t, b[r])
        if np.array_equal(a[r]["duration"], b[r]["duration"]):
            bound = SR.mel_bound(sm["cases"][case]["runs"][t]["fp64"]["feat_gen"])
            moved = float(np.abs(a[r]["feat_gen"] - b[r]["feat_gen"]).max()) / R.scale_of(a[r]["feat_gen"])
            assert moved > 100 * bound, (r, moved, bound)
    assert np.array_equal(a[1]["duration"], b[3]["duration"]) and np.array_equal(a[3]["duration"], b[1]["duration"])
    if not m.c.use_gst:
        fn = m.duration_fn(tm["fs"], tm["hop"])
        s1, s2 = fn.batch(lists, speakers=xs), fn.batch(lists, speakers=xs2)
        assert s1[0] == s2[0] and s1[2] == s2[2] and s1[1] == s2[3] and s1[3] == s2[1] and s1[1] != s2[1]


# ----------------------------------------------------------------------------------------------------------- 4. chunking
@pytest.mark.parametrize("case", SR.MODELS)
def test_speaker_rows_follow_the_lists_through_the_chunks(case):
    """Three chunks, rows 0 and 1 together, row 3 and row 2 alone: every row keeps its own x-vector -- the rows of the two-row
    chunk by their table rows, a single-row chunk on the B = 1 path with its own row of the table as the one bias."""
    from a3t_amd.engine import score_chunks
    tm = _fixture()[0]
    m = _model(case)
    lists, xs, prompt = _lists(case)
    lengths = [T for _, T in ROWS]
    cap = 2 * m.c.heads * 7 ** 2
    chunks = score_chunks(lengths, m.c.heads, cap)
    assert chunks == [[0, 1], [3], [2]] and m._chunks(lengths, cap) == chunks
    one, cut = _synth(m, lists, prompt, speakers=xs), _synth(m, lists, prompt, speakers=xs, max_score_elems=cap)
    for b, (k, T) in enumerate(ROWS):
        t = SR.tag(case, k, T)
        _check_row(case, t, cut[b])
        assert np.array_equal(one[b]["duration"], cut[b]["duration"])
        F = _fixture()[1]["cases"][case]["runs"][t]["fp64"]
        for s in SR.MEL_STAGES:
            if s in one[b]:
                err = float(np.abs(one[b][s] - cut[b][s]).max()) / R.scale_of(one[b][s])
                assert err <= SR.mel_bound(F[s]), (t, s, err)
    for b in (3, 2):        # the single-row chunks: the B = 1 path, as synthesize with that row's x-vector
        alone = _singles(case)[ROWS[b]][2]
        assert set(alone) == set(cut[b])
        for s in alone:
            assert np.array_equal(alone[s], cut[b][s]), (b, s)
    style = _style(m, prompt)
    table, rows = m.speaker_bias_table(xs)
    f1 = m.predict_frames_batch(lists, table, style=style, spk_rows=rows)
    f3 = m.predict_frames_batch(lists, table, cap, style, None, rows)
    f4 = m.predict_frames_batch(lists, table, 1, style, None, rows)           # every list alone
    for b, (k, T) in enumerate(ROWS):
        assert np.array_equal(f1[b], f3[b]) and np.array_equal(f1[b], f4[b]) and np.array_equal(f1[b], _singles(case)[(k, T)][0])
    if not m.c.use_gst:
        fn = m.duration_fn(tm["fs"], tm["hop"])
        want = fn.batch(lists, speakers=xs)
        assert fn.batch(lists, speakers=xs, max_score_elems=cap) == want
        assert [fn.with_speaker(x)(l) for l, x in zip(lists, xs)] == want
        assert fn.with_speaker(xs[1]).batch(lists, speakers=[xs[0], None, xs[2], xs[0]]) == want        # None: the callable's own


# ----------------------------------------------------------------------------------------------------- 5. NaN workspace
@pytest.mark.parametrize("case", ["xadd", "xcat"])
def test_a_nan_filled_workspace_and_random_pad_ids_change_no_valid_bit(case):
    """The per-row adds also write behind a row's length; zero_tail runs behind them, so the predictor's taps read zeros there
    whatever the padding held: pad ids 0 over a zeroed workspace against random pad ids over a NaN-filled one."""
    m = _model(case)
    lists, xs, prompt = _lists(case)
    table, rows = m.speaker_bias_table(xs)
    drows = torch.tensor(rows, dtype=torch.int32, device=DEV)
    ids0, lens = _padded(case, ROWS)
    ids1, _ = _padded(case, ROWS, pad=np.random.RandomState(9))
    assert not np.array_equal(ids0, ids1)
    dl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    m.forward_ids_batch(torch.from_numpy(ids0).to(DEV), dl, table, None, None, drows)
    m.synthesize_batch(lists, speakers=xs)                                    # (allocates every buffer of these shapes)
    torch.cuda.synchronize()
    fwd, syn = [], []
    for ids, fill in ((ids0, 0.0), (ids1, NAN)):
        for t in m.ws.bufs.values():
            t.fill_(fill) if t.is_floating_point() else t.fill_(0 if fill == 0.0 else 1 << 40)
        _, logd, frames = m.forward_ids_batch(torch.from_numpy(ids).to(DEV), dl, table, None, None, drows)
        torch.cuda.synchronize()
        fwd.append((logd.cpu().numpy().copy(), frames.cpu().numpy().copy()))
        for t in m.ws.bufs.values():
            t.fill_(fill) if t.is_floating_point() else t.fill_(0 if fill == 0.0 else 1 << 40)
        syn.append(_synth(m, lists, None, speakers=xs))
    for b, n in enumerate(lens):
        assert np.isfinite(fwd[1][0][b, :n]).all()
        assert np.array_equal(fwd[0][0][b, :n].view(np.int32), fwd[1][0][b, :n].view(np.int32)), (b, n)
        assert np.array_equal(fwd[0][1][b, :n], fwd[1][1][b, :n]), (b, n)
    for a, b in zip(*syn):
        for k in a:
            assert np.isfinite(b[k]).all() and np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------ 6. GST
def test_gst_prompts_and_speakers_are_independent_lists():
    tm = _fixture()[0]
    m = _model("gst_norm")
    ids, spk, _, _, _ = _inputs("gst_norm")
    a, b = spk[0], spk[1]
    p, q = GR.waveform(39217, seed=1), GR.waveform(30011, seed=2)
    lists = [SR.phones(tm, ids[7]), SR.phones(tm, ids[33]), SR.phones(tm, ids[7])]
    fn = m.duration_fn(tm["fs"], tm["hop"])
    assert fn.needs_prompt and fn.takes_speaker
    got = fn.batch(lists, prompts=[p, q, p], speakers=[a, a, b])
    for g, l, w, x in zip(got, lists, (p, q, p), (a, a, b)):
        assert g == fn.with_prompt(w).with_speaker(x)(l)
        assert g == fn.with_speaker(x).with_prompt(w)(l)
    # the callable's own x-vector behind None, and the prompt-bound callable's batch
    fa = m.duration_fn(tm["fs"], tm["hop"], spembs=a)
    assert fa.batch(lists, prompts=[p, q, p], speakers=[None, None, b]) == got
    assert fa.with_prompt(p).batch([lists[0], lists[2]], speakers=[None, b]) == [got[0], got[2]]
    assert fa.batch(lists, prompts=[p, q, p])[:2] == got[:2]


# --------------------------------------------------------------------------------------------------------------- 7. editor
def test_edit_batch_with_a_speaker_per_request():
    """Three requests, two speakers: one .batch call on the duration model and one copy to the host for the planning; every
    plan is the request's own, and with rows="alone" every row is edit(r, spembs=r.spembs) within the bounds of
    tests/test_gpu_sedit_rows_alone.py::test_edit_batch_rows_alone_against_edit (feat 1e-3, waveforms 2e-3 of scale)."""
    import mlm_rows_alone_ref as A
    import test_gpu_sedit_batch as SB
    from a3t_amd import sedit
    ed, oc = SB._editor()[:2]
    spk = _inputs("xadd")[1]
    reqs = [replace(r, spembs=x) for r, x in zip(SB._requests()[:3], (spk[0], spk[1], spk[0]))]
    native = _model("xadd").duration_fn(oc.fs, oc.hop_length)
    calls = {"batch": 0, "plain": 0}

    def counted(phns):
        calls["plain"] += 1
        return native(phns)

    def counted_batch(lists, **kw):
        calls["batch"] += 1
        assert [id(x) for x in kw["speakers"]].count(id(spk[1])) >= 1 and len(kw["speakers"]) == len(lists)
        return native.batch(lists, **kw)
    counted.batch, counted.takes_speaker, counted.with_speaker = counted_batch, True, native.with_speaker
    ed.duration_fn = counted
    n = {"down": 0}
    orig = torch.Tensor.cpu

    def counting(self, *a, **k):
        n["down"] += 1
        return orig(self, *a, **k)
    torch.Tensor.cpu = counting
    try:
        plans, _ = sedit.plan_batch(reqs, ed.fs, ed.hop, counted, ed.token_id_fn)
    finally:
        torch.Tensor.cpu = orig
    assert calls == {"batch": 1, "plain": 0} and n["down"] == 1
    for r, p in zip(reqs, plans):
        ms, me, op, nph, rep, add = sedit.get_phns_and_spans(r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str)
        one = sedit.prepare_features_with_duration(r.wav_org, ed.fs, ed.hop, ms, me, op, nph, rep, add, sedit.bind_request(native, r),
                                                   r.new_str, **SB._opts(r))
        assert np.array_equal(p.wav, one[0]) and list(p.phns) == list(one[1])
        assert list(p.align_start) == list(one[2]) and list(p.align_end) == list(one[3])
        assert list(p.old_span_boundary) == list(one[4]) and list(p.new_span_boundary) == list(one[5])
    # the same request under the other speaker is another plan
    other, _ = sedit.plan_batch([replace(reqs[0], spembs=spk[1])], ed.fs, ed.hop, native, ed.token_id_fn)
    assert len(other[0].wav) != len(plans[0].wav) or other[0].align_end != plans[0].align_end
    ones = [ed.edit(*SB._args(r), **SB._opts(r), spembs=r.spembs) for r in reqs]
    z = [SB._Vocoder.noise(o["feat"].shape[0], oc.hop_length) for o in ones]
    calls.update(batch=0, plain=0)
    got = ed.edit_batch(reqs, z=z, rows="alone")
    assert calls == {"batch": 1, "plain": 0}
    for i, (g, o, p) in enumerate(zip(got, ones, plans)):
        assert g["old_span_boundary"] == o["old_span_boundary"] == p.old_span_boundary
        assert g["new_span_boundary"] == o["new_span_boundary"] == p.new_span_boundary
        assert g["feat"].shape == o["feat"].shape
        np.testing.assert_allclose(g["feat"].cpu().numpy(), o["feat"].cpu().numpy(), atol=A.MEL_BOUND, rtol=A.MEL_BOUND)
        atol = 2e-3 * max(1.0, float(np.abs(o["prediction"]).max()))
        for k in ("prediction", "orgin_replaced"):
            assert g[k].shape == o[k].shape, k
            np.testing.assert_allclose(g[k], o[k], atol=atol, rtol=0)


# ------------------------------------------------------------------------------------------------------ 8. unchanged paths
@pytest.mark.parametrize("case", ["xadd", "xcat"])
def test_the_one_bias_path_is_untouched(case, monkeypatch):
    """spembs= (one x-vector for the call) launches what it launched: a3t_bias_act / the GEMM's own bias, never the per-row
    add; its results are the fixture's, and speakers=[x] * n agrees with it within the bound (the table path may round the
    concat projection's last bit differently: the bias is added behind the GEMM, not in its epilogue)."""
    from a3t_amd import ops
    tm, sm, _ = _fixture()
    m = _model(case)
    ids, spk, prompt, _, _ = _inputs(case)
    rows = tuple((0, T) for _, T in ROWS)
    lists, _, _ = _lists(case, rows)
    seen = []
    real = ops.gst_add_style
    monkeypatch.setattr(ops, "gst_add_style", lambda *a, **k: (seen.append("rows"), real(*a, **k))[1])
    fn = m.duration_fn(tm["fs"], tm["hop"], spembs=spk[0])
    one = _synth(m, lists, prompt, spembs=spk[0])
    secs = fn.batch(lists)
    assert not seen
    tab = _synth(m, lists, prompt, speakers=[spk[0]] * len(lists))
    assert fn.batch(lists, speakers=[None] * len(lists)) == secs == fn.batch(lists, speakers=[spk[0]] * len(lists))
    assert seen
    for b, (k, T) in enumerate(rows):
        t = SR.tag(case, k, T)
        _check_row(case, t, one[b])
        _check_row(case, t, tab[b])
        assert np.array_equal(one[b]["duration"], tab[b]["duration"])
        F = sm["cases"][case]["runs"][t]["fp64"]
        for s in SR.MEL_STAGES:
            if s in one[b]:
                err = float(np.abs(one[b][s] - tab[b][s]).max()) / R.scale_of(one[b][s])
                assert err <= SR.mel_bound(F[s]), (t, s, err)
