"""Host-side checks of the batched duration path: which phone lists an edit asks the duration model for
(sedit.duration_queries), plan_batch's single `.batch` call, and the CPU restatement of the ragged forward
(tests/fs2_ragged_ref.py) against the reference's own outputs in tests/golden/fs2_duration.npz.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import fs2_ragged_ref as R

G = os.path.join(os.path.dirname(__file__), "golden")


def _sedit_cases():
    return json.load(open(os.path.join(G, "sedit.json")))


def _fake_seconds(phns):
    """A deterministic stand-in for a duration model: seconds that depend on the phone and its position."""
    return [0.03 + 0.01 * ((sum(map(ord, ph)) + 3 * i) % 11) for i, ph in enumerate(phns)]


# ------------------------------------------------------------------------------------------------- duration_queries
@pytest.mark.parametrize("variant", ["own", "mask_reconstruct", "start_end_sp"])
def test_duration_queries_equal_what_the_plan_asks_for(variant):
    from a3t_amd import sedit
    fx = _sedit_cases()
    assert len(fx["cases"]) == 40
    seen = set()
    for case in fx["cases"]:
        opts = dict(case["opts"])
        if variant != "own":
            opts[variant] = True
        args = (case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"], case["old_str"], case["new_str"])
        ms, me, op, nph, rep, add = sedit.get_phns_and_spans(*args)
        asked = []

        def recording(phns):
            asked.append(list(phns))
            return _fake_seconds(phns)
        wav = np.zeros(int(np.ceil(me[-1] * fx["fs"])) + fx["hop"], np.float32)
        sedit.prepare_features_with_duration(wav, fx["fs"], fx["hop"], list(ms), list(me), list(op), list(nph), rep, add,
                                             recording, case["new_str"], **opts)
        got = sedit.duration_queries(op, nph, case["new_str"], mask_reconstruct=opts["mask_reconstruct"],
                                     start_end_sp=opts["start_end_sp"])
        assert got == asked, (case["kind"], opts)
        seen.add(len(asked))
    # the three shapes of an answer all occur: nothing (own / mask_reconstruct), the old list alone, old and new
    assert seen == ({0, 2} if variant == "mask_reconstruct" else {0, 1, 2})


def test_duration_queries_leave_their_arguments_alone():
    from a3t_amd import sedit
    old, new = ["K", "AE1", "T"], ["K", "AE1", "T", "S"]
    q = sedit.duration_queries(old, new, "cats", start_end_sp=True)
    assert q == [["K", "AE1", "T"], ["K", "AE1", "T", "S", "sp"]] and new == ["K", "AE1", "T", "S"]
    assert sedit.duration_queries(old, new + ["sp"], "cats", start_end_sp=True)[1] == new + ["sp"]


# ------------------------------------------------------------------------------------------------------- plan_batch
def _samples(fx, case):
    from a3t_amd import sedit
    _, me, *_ = sedit.get_phns_and_spans(case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"],
                                         case["old_str"], case["new_str"])
    return int(np.ceil(me[-1] * fx["fs"])) + fx["hop"]


def _requests(n=12):
    from a3t_amd.sedit import EditRequest
    fx = _sedit_cases()
    reqs = []
    for case in fx["cases"][:n]:
        wav = (0.01 * np.arange(_samples(fx, case)) % 1.0).astype(np.float32)
        reqs.append(EditRequest(wav, case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"],
                                case["old_str"], case["new_str"], **case["opts"]))
    return fx, reqs


def _ids(phns):
    return np.array([2 + sum(map(ord, ph)) % 60 for ph in phns], dtype=np.int64)


def test_plan_batch_asks_a_batched_duration_model_once():
    from a3t_amd import sedit
    fx, reqs = _requests()
    plain_calls = []

    def plain(phns):
        plain_calls.append(tuple(phns))
        return _fake_seconds(phns)
    want_plans, want_data = sedit.plan_batch(reqs, fx["fs"], fx["hop"], plain, _ids)
    assert len(plain_calls) == len(set(plain_calls)) >= 2

    calls = {"plain": 0, "batch": []}

    def batched(phns):
        calls["plain"] += 1
        return _fake_seconds(phns)

    def batch(lists):
        calls["batch"].append([tuple(x) for x in lists])
        return [_fake_seconds(x) for x in lists]
    batched.batch = batch
    plans, data = sedit.plan_batch(reqs, fx["fs"], fx["hop"], batched, _ids)
    assert calls["plain"] == 0 and len(calls["batch"]) == 1
    # the distinct lists, each once, in the order a plain duration_fn meets them
    assert calls["batch"][0] == plain_calls
    assert len(plans) == len(want_plans) == len(reqs)
    for a, b in zip(plans, want_plans):
        assert a.wav.dtype == b.wav.dtype and np.array_equal(a.wav, b.wav)
        assert a.phns == b.phns and a.align_start == b.align_start and a.align_end == b.align_end
        assert list(a.old_span_boundary) == list(b.old_span_boundary)
        assert list(a.new_span_boundary) == list(b.new_span_boundary)
    for (ka, da), (kb, db) in zip(data, want_data):
        assert ka == kb and set(da) == set(db)
        for k in da:
            assert da[k].dtype == db[k].dtype and np.array_equal(da[k], db[k]), k


def test_plan_batch_with_nothing_to_predict_makes_no_batch_call():
    """`[MASK]` + mask_reconstruct needs no durations: an empty question is not put to the model."""
    from a3t_amd import sedit
    from a3t_amd.sedit import EditRequest
    fx = _sedit_cases()
    case = [c for c in fx["cases"] if c["kind"] == "mask_rec"][0]
    wav = np.zeros(_samples(fx, case), np.float32)
    req = EditRequest(wav, case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"], case["old_str"],
                      case["new_str"], **case["opts"])

    def fn(phns):
        raise AssertionError("no duration is needed")
    fn.batch = fn
    plans, _ = sedit.plan_batch([req], fx["fs"], fx["hop"], fn, _ids)
    assert len(plans) == 1


# ---------------------------------------------------------------------- the ragged restatement against the reference
@pytest.mark.parametrize("case", ["lj", "lj_xadd", "lj_xcat", "small_c384"])
def test_ragged_restatement_against_reference(case):
    """One padded batch of the fixture's five lengths per model.  Log domain <= 1e-4 (the bound tests/test_gpu_duration.py
    uses against the same fixture; measured on the CPU: 4.1e-6); frames equal wherever the reference's exp(x) - 1 is more than
    1e-3 from a .5 tie, a rule that leaves out at most one element per row of this fixture."""
    m, z = R.meta(), R.arrays()
    cfg, p = R.checkpoint(m, case)
    ids, lens = R.fixture_batch(z, m, case)
    spk = z[f"{case}.spembs"] if f"{case}.spembs" in z else None
    with torch.no_grad():
        hs, logd = R.ragged_forward(p, cfg["tts_conf"], ids, lens, spk)
    frames = R.frames_of(logd).numpy()
    logd = logd.numpy()
    for b, T in enumerate(lens):
        pre = f"{case}.T{T}."
        err = np.abs(logd[b, :T] - z[pre + "logd"]).max()
        print(f"{case} T={T}: max |dlogd| {err:.3g}")
        assert err <= 1e-4, (T, err)
        far = R.tie_distance(z[pre + "expm1"]) > 1e-3
        assert far.sum() >= T - 1, (T, int(far.sum()))
        assert np.array_equal(frames[b, :T][far], z[pre + "frames"][far]), T
        assert np.abs(frames[b, :T] - z[pre + "frames"]).max() <= 1
        if T == m["hs_length"]:
            ref = z[pre + "hs"]
            assert np.abs(hs[b, :T].numpy() - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


def test_plain_padded_batch_is_not_the_row_alone():
    """Why the lengths are needed: the same restatement told that every row is Tmax long (a plain padded batch whose keys are
    not even masked is the mildest version of it) misses the reference on the short rows by far more than the bound."""
    m, z = R.meta(), R.arrays()
    cfg, p = R.checkpoint(m, "small_c384")
    ids, lens = R.fixture_batch(z, m, "small_c384")
    ids, lens = ids[:3, :33], lens[:3]
    with torch.no_grad():
        _, good = R.ragged_forward(p, cfg["tts_conf"], ids, lens)
        _, bad = R.ragged_forward(p, cfg["tts_conf"], ids, [33, 33, 33])
    for b, T in enumerate(lens):
        ref = z[f"small_c384.T{T}.logd"]
        assert np.abs(good[b, :T].numpy() - ref).max() <= 1e-4
        if T < 33:
            assert np.abs(bad[b, :T].numpy() - ref).max() > 1e-2


# ------------------------------------------------------------------------------------------- the model's host logic
def _cpu_model(case="small_c384"):
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
    cfg, p = R.checkpoint(R.meta(), case)
    return FS2DurationModel(FS2DurationConfig.from_espnet(cfg), "cpu").load_state_dict({"tts." + k: v for k, v in p.items()})


def test_chunks_sort_by_length_and_respect_the_cap():
    m = _cpu_model()
    H = m.c.heads
    lengths = [40, 3, 17, 40, 9, 120, 5]
    one = m._chunks(lengths, 1 << 24)
    assert one == [[1, 6, 4, 2, 0, 3, 5]]
    cap = 3 * H * 40 * 40
    chunks = m._chunks(lengths, cap)
    assert sorted(i for ch in chunks for i in ch) == list(range(len(lengths)))
    assert [lengths[i] for ch in chunks for i in ch] == sorted(lengths)
    assert len(chunks) >= 2
    for ch in chunks:
        assert len(ch) == 1 or len(ch) * H * lengths[ch[-1]] ** 2 <= cap
    assert m._chunks(lengths, 1) == [[i] for i in one[0]]      # nothing fits: every list alone


def test_duration_fn_has_a_batch_attribute():
    fn = _cpu_model().duration_fn(24000, 300)
    assert callable(fn) and callable(fn.batch)
    assert fn.batch([]) == []


def test_engine_refuses_lens_outside_fp32_eval():
    """lens needs fp32 compute, eval mode, forward only; the check comes before any kernel."""
    from a3t_amd.engine import MLMEngine
    m = _cpu_model()
    lens = torch.tensor([3, 5], dtype=torch.int32)
    x = torch.zeros(2 * 5, m.c.adim)
    for kw in (dict(compute="bf16", training=False), dict(compute="f32", training=True)):
        eng = MLMEngine(m.c, m.store, **kw)
        with pytest.raises(ValueError, match="fp32 compute, eval mode"):
            eng.block_fwd("enc.0", x, eng.pe[:5], None, 2, 5, lens=lens)
    with pytest.raises(ValueError, match="int32"):
        m.eng.block_fwd("enc.0", x, m.eng.pe[:5], None, 2, 5, lens=lens.long())
