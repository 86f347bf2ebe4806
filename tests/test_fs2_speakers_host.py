"""Host-side checks of one x-vector per request (a3t_amd/duration.py speaker_bias_table / duration_fn(...).batch(speakers=),
a3t_amd/fs2_tts.py synthesize_batch(speakers=), a3t_amd/sedit.py EditRequest.spembs / bind_request / plan_batch): the torch
restatement, row by row with each row's own x-vector (tests/fs2_speakers_ref.py), against the reference's own outputs in
tests/golden/fs2_speakers.{npz,json}; the de-duplication of x-vectors by object; the planning of a batch of requests from
several speakers on a stub duration function; the refusals.  No GPU."""
import functools
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import fs2_speakers_ref as SR
import fs2_tts_ref as R
from test_sedit_batch_host import _fixture, _ids, _requests

G = os.path.join(os.path.dirname(__file__), "golden")


@functools.lru_cache(maxsize=None)
def _metas():
    return R.meta(), SR.meta()


# ------------------------------------------------------------------------------------------------- the fixture itself
def test_fixture_is_not_vacuous():
    tm, sm = _metas()
    z = SR.arrays()
    assert sm["models"] == list(SR.MODELS) and sm["lengths"] == list(SR.LENGTHS) and sm["norms"] == [0.3, 1.0, 20.0]
    assert sm["tie_margin"] >= 10 * 1e-4 * (sm["max_duration"] + 1)
    n = 0
    for case in SR.MODELS:
        ids, spk, _, _, _ = SR.inputs(tm, sm, case)
        assert [round(float(np.linalg.norm(x)), 4) for x in spk] == sm["norms"]
        for k in range(SR.N_SPEAKERS):
            for T in SR.LENGTHS:
                t = SR.tag(case, k, T)
                run = sm["cases"][case]["runs"][t]
                d = z[t + ".duration"]
                assert d.shape == (T,) and d.max() <= sm["max_duration"] and run["tie"] >= sm["tie_margin"], t
                assert z[t + ".feat_gen"].shape == (run["frames"], 80) == (int(d.sum()), 80), t
                assert ((t + ".feat_gen_denorm") in z) == tm["cases"][case]["normalize"]
                n += 1
        # any two x-vectors of a model differ in what they give, at every length
        for T in SR.LENGTHS:
            for a in range(SR.N_SPEAKERS):
                for b in range(a + 1, SR.N_SPEAKERS):
                    da, db = z[SR.tag(case, a, T) + ".duration"], z[SR.tag(case, b, T) + ".duration"]
                    sep = sm["cases"][case]["separation"][f"T{T}.s{a}.s{b}"]
                    assert (sep == "durations" and not np.array_equal(da, db)) or sep > 100 * 1e-4
    assert n == 27
    for f in ("fs2_speakers.npz", "fs2_speakers.json"):
        assert os.path.getsize(os.path.join(G, f)) < (1 << 20), f


# ------------------------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("case", SR.MODELS)
def test_restatement_row_by_row_against_the_reference(case):
    """Every (x-vector, length) of a model as a row of its own: durations exact, every stage within max(4 F, 1e-5) of scale, F
    the reference's own fp32-vs-fp64 distance of that stage (fp64 restatement, as tests/test_fs2_tts_host.py)."""
    tm, sm = _metas()
    z = SR.arrays()
    cfg, p = R.checkpoint(tm, case)
    ids, spk, prompt, mean, std = SR.inputs(tm, sm, case)
    pairs = [(k, T) for k in range(SR.N_SPEAKERS) for T in SR.LENGTHS]
    rows = SR.synthesize_rows(p, cfg["tts_conf"], [ids[T] for _, T in pairs], [spk[k] for k, _ in pairs], prompt, mean, std)
    for (k, T), got in zip(pairs, rows):
        t = SR.tag(case, k, T)
        run = sm["cases"][case]["runs"][t]
        assert np.array_equal(got["duration"], z[t + ".duration"]), t
        assert got["feat_gen"].shape[0] == run["frames"]
        for s in SR.STAGES:
            if f"{t}.{s}" not in z:
                assert s == "feat_gen_denorm"
                continue
            want, F = z[f"{t}.{s}"], run["fp64"][s]
            err = float(np.abs(got[s] - want).max()) / R.scale_of(want)
            print(f"{t} {s}: err {err:.2e} of scale, F {F:.2e}")
            assert err <= max(4 * F, 1e-5), (t, s, err, F)


# ------------------------------------------------------------------------------------------ models on the host, fake ops
@functools.lru_cache(maxsize=None)
def _cpu_model(case):
    from a3t_amd.fs2_tts import FS2TTSConfig, FS2TTSModel
    cfg, p = R.checkpoint(_metas()[0], case)
    c = FS2TTSConfig.from_espnet(cfg, gst=bool(cfg["tts_conf"].get("use_gst")))
    return FS2TTSModel(c, "cpu").load_state_dict({"tts." + k: v for k, v in p.items()})


@pytest.fixture
def fake_ops(monkeypatch):
    """a3t_amd.ops.l2_normalize / linear_fwd in torch, recording the shapes they were called with."""
    from a3t_amd import ops
    calls = []

    def l2_normalize(x, y, eps=1e-12):
        calls.append(("l2_normalize", tuple(x.shape)))
        y.copy_(torch.nn.functional.normalize(x, dim=1, eps=eps))

    def linear_fwd(x, W, out, bias=None, **kw):
        calls.append(("linear_fwd", tuple(x.shape), tuple(W.shape)))
        out.copy_(torch.nn.functional.linear(x, W, bias))
    monkeypatch.setattr(ops, "l2_normalize", l2_normalize)
    monkeypatch.setattr(ops, "linear_fwd", linear_fwd)
    return calls


def test_speaker_bias_table_finds_distinct_vectors_by_object(fake_ops):
    tm, sm = _metas()
    m = _cpu_model("xcat")
    a, b, c = SR.inputs(tm, sm, "xcat")[1]
    table, rows = m.speaker_bias_table([a, b, a, c])
    assert rows == [0, 1, 0, 2] and table.shape == (3, m.c.adim)
    assert fake_ops == [("l2_normalize", (3, 512)), ("linear_fwd", (3, 512), (m.c.adim, 512))]       # one of each, M = S
    _, p = R.checkpoint(tm, "xcat")
    for r, x in enumerate((a, b, c)):
        s = torch.nn.functional.normalize(torch.from_numpy(x)[None])
        want = torch.nn.functional.linear(s, p["projection.weight"][:, m.c.adim:], p["projection.bias"])
        assert torch.allclose(table[r:r + 1], want, atol=1e-6)
        # the S = 1 case is a row of the table (to the host BLAS's rounding here; bit for bit on the device, see the GPU tests)
        assert torch.allclose(table[r:r + 1], m.speaker_bias(x), atol=1e-6)
    # an equal copy is another object: identity, as batch(..., prompts=) finds distinct prompts
    assert m.speaker_bias_table([a, a.copy()])[1] == [0, 1]
    # first-use order
    assert m.speaker_bias_table([c, a, c, b, a])[1] == [0, 1, 0, 2, 1]
    with pytest.raises(ValueError, match=r"spembs has 511 values, the checkpoint expects 512 \(x-vector 2\)"):
        m.speaker_bias_table([a, b, a[:511]])
    with pytest.raises(ValueError, match="no x-vector projection"):
        _cpu_model("plain").speaker_bias_table([a])


def test_duration_fn_interface_and_refusals(fake_ops):
    tm, sm = _metas()
    fs, hop = tm["fs"], tm["hop"]
    a, b, _ = SR.inputs(tm, sm, "xadd")[1]
    lists = [["HH", "AH0"], ["sp", "L", "OW1"]]
    x = _cpu_model("xadd").duration_fn(fs, hop)
    assert x.takes_speaker is True and callable(x.with_speaker) and not getattr(x, "needs_prompt", False)
    bound = x.with_speaker(a)
    assert callable(bound) and callable(bound.batch) and bound.takes_speaker
    with pytest.raises(ValueError, match="speakers: 1 x-vectors for 2 phone lists"):
        x.batch(lists, speakers=[a])
    with pytest.raises(ValueError, match=r"speakers\[1\] is None"):
        x.batch(lists, speakers=[a, None])
    with pytest.raises(ValueError, match=r"x-vector 1"):
        x.batch(lists, speakers=[a, b[:100]])
    assert x.batch([], speakers=[]) == []
    plain = _cpu_model("plain").duration_fn(fs, hop)
    assert not hasattr(plain, "takes_speaker") and not hasattr(plain, "with_speaker")
    with pytest.raises(ValueError, match="speakers= given, but this checkpoint has no x-vector projection"):
        plain.batch(lists, speakers=[a, b])
    g = _cpu_model("gst_norm").duration_fn(24000, hop)
    assert g.needs_prompt and g.takes_speaker
    ga = g.with_speaker(a)
    assert ga.needs_prompt and callable(ga.with_prompt) and ga.takes_speaker
    wav = np.zeros(24000, np.float32)
    gp = g.with_prompt(wav)
    assert gp.takes_speaker and callable(gp.with_speaker(b)) and callable(gp.with_speaker(b).batch)
    with pytest.raises(ValueError, match="prompts"):
        g.batch(lists, speakers=[a, b])
    with pytest.raises(ValueError, match="speakers: 3 x-vectors for 2 phone lists"):
        g.batch(lists, prompts=[wav, wav], speakers=[a, b, a])


def test_synthesize_batch_refusals():
    tm, sm = _metas()
    a, b, _ = SR.inputs(tm, sm, "xadd")[1]
    m = _cpu_model("xadd")
    lists = [["HH", "AH0"], ["sp", "L", "OW1"]]
    with pytest.raises(ValueError, match="spembs .*speakers"):
        m.synthesize_batch(lists, spembs=a, speakers=[a, b])
    with pytest.raises(ValueError, match="spembs .*speakers"):
        m.synthesize_ids_batch([[3, 4], [5]], a, speakers=[a, b])
    with pytest.raises(ValueError, match="speakers: 3 x-vectors for 2 phone lists"):
        m.synthesize_batch(lists, speakers=[a, b, a])
    with pytest.raises(ValueError, match=r"speakers\[0\] is None"):
        m.synthesize_batch(lists, speakers=[None, b])
    with pytest.raises(ValueError, match="x-vector 1"):
        m.synthesize_batch(lists, speakers=[a, b[:7]])
    with pytest.raises(ValueError, match="no x-vector projection"):
        _cpu_model("plain").synthesize_batch(lists, speakers=[a, b])
    with pytest.raises(ValueError, match="needs spembs"):
        m.synthesize_batch(lists)


# ------------------------------------------------------------------------------------------------------ the planning
def _scale(spk):
    return 1.0 if spk is None else 1.0 + float(np.asarray(spk).reshape(-1)[0])


def _stub(dur, own=None, with_batch=True, prompted=False):
    """A duration function whose answers depend on the speaker (and, prompted, on the prompt's length), with the interface of
    FS2DurationModel.duration_fn; log: the arguments of every .batch call, asked: every (speaker, list) a plain call answered."""
    log, asked = [], []

    def answer(phns, spk, wav):
        # (not one factor for all phones: duration_adjust would divide it out again)
        k = (_scale(spk) - 1.0) * (1.0 if wav is None else 1.0 + 1e-6 * len(wav))
        return [(1.0 + k * (i % 3)) * d for i, d in enumerate(dur(list(phns)))]

    def make(spk, wav=None):
        def fn(phns):
            if prompted and wav is None:
                raise ValueError("needs a prompt")
            asked.append((spk, tuple(phns)))
            return answer(phns, spk, wav)
        if with_batch:
            def batch(lists, **kw):
                log.append((list(lists), kw))
                n = len(lists)
                sp, pr = kw.get("speakers") or [None] * n, kw.get("prompts") or [wav] * n
                assert len(sp) == len(pr) == n and not (prompted and any(w is None for w in pr))
                return [answer(l, spk if s is None else s, w) for l, s, w in zip(lists, sp, pr)]
            fn.batch = batch
        fn.takes_speaker = True
        fn.with_speaker = lambda x: make(x, wav)
        if prompted:
            fn.needs_prompt = wav is None
            fn.with_prompt = lambda w: make(spk, w)
        return fn
    return make(own), log, asked


def _plan_alone(sedit, r, fn, fs, hop):
    ms, me, op, nph, rep, add = sedit.get_phns_and_spans(r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str)
    return sedit.prepare_features_with_duration(np.asarray(r.wav_org, np.float32), fs, hop, ms, me, op, nph, rep, add, fn,
                                                r.new_str, mask_reconstruct=r.mask_reconstruct,
                                                duration_adjust=r.duration_adjust, start_end_sp=r.start_end_sp)


def _same_plan(p, one):
    assert np.array_equal(p.wav, np.asarray(one[0])) and list(p.phns) == list(one[1])
    assert list(p.align_start) == list(one[2]) and list(p.align_end) == list(one[3])
    assert list(p.old_span_boundary) == [int(x) for x in one[4]] and list(p.new_span_boundary) == [int(x) for x in one[5]]


def _speaker_requests():
    fx, waves, dur = _fixture()
    (rep, mask, app, dele), _ = _requests(fx, waves)
    a, b = np.array([0.25], np.float32), np.array([0.5], np.float32)
    # one speaker twice with the same lists, the same lists under another speaker, other lists, and a request without spembs
    reqs = [replace(rep, spembs=a), replace(rep, spembs=a), replace(rep, spembs=b), replace(mask, spembs=a),
            replace(app, spembs=b), dele]
    return fx, dur, reqs, a, b


@pytest.mark.parametrize("prompted", [False, True])
def test_plan_batch_asks_once_with_one_speaker_per_query(prompted):
    from a3t_amd import sedit
    fx, dur, reqs, a, b = _speaker_requests()
    fs, hop = fx["fs"], fx["hop"]
    own = np.array([0.125], np.float32)
    fn, log, asked = _stub(dur, own, prompted=prompted)
    plans, data = sedit.plan_batch(reqs, fs, hop, fn, _ids)
    assert len(log) == 1 and not asked                                   # exactly one .batch call, no plain call
    lists, kw = log[0]
    assert set(kw) == ({"speakers", "prompts"} if prompted else {"speakers"})
    speakers = kw["speakers"]
    assert len(speakers) == len(lists) and all(s is None or s is a or s is b for s in speakers)
    # the queries: what every request asks, each (speaker object, [request if prompted,] list) once, in first-use order
    want = []
    for i, r in enumerate(reqs):
        _, _, old_phns, phns, _, _ = sedit.get_phns_and_spans(r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str,
                                                              r.new_str)
        for q in sedit.duration_queries(old_phns, phns, r.new_str, r.mask_reconstruct, r.start_end_sp):
            key = (id(r.spembs) if r.spembs is not None else None, i if prompted else None, tuple(q))
            if key not in [k for k, _ in want]:
                want.append((key, r))
    got = [(id(s) if s is not None else None, tuple(l)) for s, l in zip(speakers, lists)]
    assert got == [(k[0], k[2]) for k, _ in want]
    if prompted:
        assert all(w is r.wav_org for w, (_, r) in zip(kw["prompts"], want))
    else:
        assert len(set(got)) == len(got)
        # requests 0 and 1 (one speaker object, the same lists) share their queries; request 2 (another speaker) asks again
        rep_lists = {tuple(l) for s, l in zip(speakers, lists) if s is a} & {tuple(l) for s, l in zip(speakers, lists) if s is b}
        assert len(rep_lists) == 2 and sum(1 for s in speakers if s is None) >= 1
        assert sum(1 for s, l in zip(speakers, lists) if s is a and tuple(l) in rep_lists) == 2
    # every plan is the plan of the request alone, bound to its speaker (and prompt)
    for r, p in zip(reqs, plans):
        alone = fn.with_prompt(r.wav_org) if prompted else fn
        alone = alone if r.spembs is None else alone.with_speaker(r.spembs)
        _same_plan(p, _plan_alone(sedit, r, alone, fs, hop))
        _same_plan(p, _plan_alone(sedit, r, sedit.bind_request(fn, r), fs, hop))
    # the speaker decides: the same request under the other speaker plans another waveform
    assert len(plans[0].wav) == len(plans[1].wav) != len(plans[2].wav)


def test_plan_batch_without_a_batch_attribute_binds_every_request():
    from a3t_amd import sedit
    fx, dur, reqs, a, b = _speaker_requests()
    fn, log, asked = _stub(dur, np.array([0.125], np.float32), with_batch=False)
    plans, _ = sedit.plan_batch(reqs, fx["fs"], fx["hop"], fn, _ids)
    assert not log and len(asked) == len({(id(s) if s is not None else None, l) for s, l in asked})
    for r, p in zip(reqs, plans):
        _same_plan(p, _plan_alone(sedit, r, sedit.bind_request(fn, r), fx["fs"], fx["hop"]))


def test_requests_without_spembs_see_the_old_call():
    """No request carries spembs: the .batch of the duration function is called as before, with the lists alone (a stub whose
    .batch takes no speakers keyword at all), and a prompted one with prompts= only."""
    from a3t_amd import sedit
    fx, waves, dur = _fixture()
    reqs, _ = _requests(fx, waves)
    seen = []

    def fn(phns):
        raise AssertionError("a plain call")

    def batch(lists):
        seen.append(list(lists))
        return [dur(l) for l in lists]
    fn.batch = batch
    plans, _ = sedit.plan_batch(reqs, fx["fs"], fx["hop"], fn, _ids)
    assert len(seen) == 1
    for r, p in zip(reqs, plans):
        _same_plan(p, _plan_alone(sedit, r, dur, fx["fs"], fx["hop"]))

    def pbatch(lists, prompts):
        seen.append((list(lists), prompts))
        return [dur(l) for l in lists]
    fn.batch, fn.needs_prompt, fn.with_prompt = pbatch, True, lambda w: dur
    sedit.plan_batch(reqs, fx["fs"], fx["hop"], fn, _ids)
    assert len(seen) == 2 and len(seen[1][1]) == len(seen[1][0])


def test_spembs_against_a_plain_callable_is_refused_before_anything_is_predicted():
    from a3t_amd import sedit
    fx, waves, dur = _fixture()
    reqs, _ = _requests(fx, waves)
    calls = []

    def plain(phns):
        calls.append(tuple(phns))
        return dur(phns)
    x = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="request 1 brings spembs"):
        sedit.plan_batch([reqs[0], replace(reqs[1], spembs=x)], fx["fs"], fx["hop"], plain, _ids)
    with pytest.raises(ValueError, match="takes no speaker"):
        sedit.bind_request(plain, replace(reqs[0], spembs=x))
    assert not calls
    assert sedit.bind_request(plain, reqs[0]) is plain
    # the field is the last one: positional construction is what it was
    from dataclasses import fields
    assert [f.name for f in fields(sedit.EditRequest)][-2:] == ["dynamic_eval", "spembs"] and reqs[0].spembs is None

    class _FE:
        fs, hop_length = fx["fs"], fx["hop"]

    class _Coll:
        feats_extract = _FE()
    ed = sedit.SpeechEditor(object(), _Coll(), None, _ids, plain)
    r = reqs[0]
    with pytest.raises(ValueError, match="takes no speaker"):
        ed.decode(r.wav_org, r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str, spembs=x)
    with pytest.raises(ValueError, match="takes no speaker"):
        ed.edit(r.wav_org, r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str, spembs=x)
    assert not calls
