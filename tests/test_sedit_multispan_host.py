"""Host half of multi-span speech editing: get_phns_and_multi_spans / prepare_features_multi against the single-span functions
on the recorded edits, a request with two separate edits (kept phones, waveform pieces, gaps, the collate's mask), the planner's
merging rules, span_windows, replace_waveform_multi and the two new C ABI entries.  No GPU.  Requests: tests/sedit_multispan_ref.py."""
import difflib
import math
import os
import re
from dataclasses import replace

import numpy as np
import pytest
import torch

import sedit_multispan_ref as M
from oracle import a3t_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("replace", "mask", "append", "delete")


def _ids(phns):
    return np.array([2 + sum(map(ord, ph)) % 36 for ph in phns], dtype=np.int64)


def _runs(case_or_request):
    """The changed runs of the word diff the planner is specified with."""
    from a3t_amd.sedit import _parse_keys
    c = case_or_request if isinstance(case_or_request, dict) else vars(case_or_request)
    old = [w for _, w in _parse_keys(c["word2phns"]) if w != "sp"]
    new = [w for _, w in _parse_keys(c["new_word2phns"])]
    return [o for o in difflib.SequenceMatcher(None, old, new, autojunk=False).get_opcodes() if o[0] != "equal"]


def _same(a, b):
    assert len(a) == len(b) == 6
    assert np.array_equal(np.asarray(a[0]), np.asarray(b[0])) and np.asarray(a[0]).dtype == np.asarray(b[0]).dtype
    for x, y in zip(a[1:], b[1:]):
        assert list(x) == list(y)


# ------------------------------------------------------------------------------------------------- single-run equivalence
def test_recorded_edits_with_one_changed_run_plan_as_before():
    """All 40 recorded edits through get_phns_and_multi_spans(max_spans=3) + prepare_features_multi.  An edit with at most one
    changed run, an append and a `[MASK]` request give what get_phns_and_spans + prepare_features_with_duration give, `==` on
    every output, and so the reference driver's recorded plan.  Two of the recorded edits (a `replace` whose fresh words repeat
    a kept word, a `first` that inserts around a kept word) have two changed runs under the word diff: for those the
    single-span result is what max_spans=1 gives, and max_spans=3 plans more than one span (they are counted, so that the
    fixture cannot drift into checking nothing)."""
    from a3t_amd import sedit
    fx, waves, dur = M.fixture()
    fs, hop = fx["fs"], fx["hop"]
    assert len(fx["cases"]) == 40
    multi = 0
    for c in fx["cases"]:
        wav = waves[c["wav"] + ".in"]
        args = (c["times2"], c["word2phns"], c["new_phns"], c["new_word2phns"], c["old_str"], c["new_str"])
        spans1 = sedit.get_phns_and_spans(*args)
        plan1 = sedit.prepare_features_with_duration(wav, fs, hop, *spans1, dur, c["new_str"], **c["opts"])
        single = len(_runs(c)) <= 1 or c["old_str"] == c["new_str"][:len(c["old_str"])] or "[MASK]" in c["new_str"]
        for ms in ((3,) if single else (1,)):
            spans = sedit.get_phns_and_multi_spans(*args, max_spans=ms)
            assert len(spans) == 6 and all(list(x) == list(y) for x, y in zip(spans, spans1))
            plan = sedit.prepare_features_multi(wav, fs, hop, *spans, dur, c["new_str"], **c["opts"])
            _same(plan, plan1)
            assert plan[4] == c["plan"]["old_span_boundary"] and plan[5] == c["plan"]["new_span_boundary"]
            assert np.array_equal(plan[0], waves[c["wav"] + ".out"])
        if not single:
            multi += 1
            spans = sedit.get_phns_and_multi_spans(*args, max_spans=3)
            assert len(spans[4]) == len(spans[5]) == len(_runs(c)) == 2 and isinstance(spans[4][0], list)
    assert multi == 2


def test_plan_batch_with_max_spans_equals_the_recorded_plans():
    """plan_batch on the first recorded edit of the four kinds, every request with max_spans=3: the recorded plans, the same
    duration queries, and the plan's span lists next to the boundaries."""
    from a3t_amd import sedit
    fx, waves, dur = M.fixture()
    cases = [[c for c in fx["cases"] if c["kind"] == k][0] for k in KINDS]
    assert all(len(_runs(c)) <= 1 or c["kind"] in ("mask", "append") for c in cases)
    reqs = [sedit.MultiSpanEditRequest(waves[c["wav"] + ".in"], c["times2"], c["word2phns"], c["new_phns"], c["new_word2phns"],
                              c["old_str"], c["new_str"], max_spans=3, **c["opts"]) for c in cases]
    calls3, calls1 = [], []
    plans, data = sedit.plan_batch(reqs, fx["fs"], fx["hop"], lambda p: calls3.append(tuple(p)) or dur(p), _ids)
    plans1, data1 = sedit.plan_batch([replace(r, max_spans=1) for r in reqs], fx["fs"], fx["hop"],
                                     lambda p: calls1.append(tuple(p)) or dur(p), _ids)
    assert calls3 == calls1
    for c, p, p1, (_, d), (_, d1) in zip(cases, plans, plans1, data, data1):
        assert p.old_span_boundary == c["plan"]["old_span_boundary"] and p.new_span_boundary == c["plan"]["new_span_boundary"]
        assert np.array_equal(p.wav, waves[c["wav"] + ".out"]) and list(p.phns) == c["plan"]["phns"]
        assert list(p.align_start) == c["plan"]["mfa_start"] and list(p.align_end) == c["plan"]["mfa_end"]
        assert p.old_spans == [p.old_span_boundary] == p1.old_spans and p.new_spans == [p.new_span_boundary] == p1.new_spans
        assert all(np.array_equal(d[k], d1[k]) for k in d)


# ------------------------------------------------------------------------------------------------------- two-run request
@pytest.fixture(scope="module")
def two_run():
    """BLUE SAT CAT sp MAT THE FAST MAT sp with SAT -> ZEBRA and FAST -> PLUM: CAT, MAT and THE stay between the edits."""
    from a3t_amd import sedit
    fx, waves, dur = M.fixture()
    r = M.request(fx, waves, M.SEVEN, max_spans=2, swap={1: "ZEBRA", 5: "PLUM"})
    spans = sedit.get_phns_and_multi_spans(*M.args(r), max_spans=2)
    plan = sedit.prepare_features_multi(r.wav_org, fx["fs"], fx["hop"], *spans, dur, r.new_str, **M.OPTS)
    return fx, waves, dur, r, spans, plan


def test_two_run_request_keeps_what_lies_between_the_edits(two_run):
    from a3t_amd import sedit
    fx, waves, dur, r, spans, plan = two_run
    fs, hop = fx["fs"], fx["hop"]
    words = [w for w, _ in M.old_words(fx["cases"][M.SEVEN])]
    assert words == ["BLUE", "SAT", "CAT", "MAT", "THE", "FAST", "MAT"] and len(_runs(r)) == 2
    ms, me, old_phns, new_phns, rep, add = spans
    # the premise: the single-span planner replaces the three words in the middle too
    rep1, add1 = sedit.get_phns_and_spans(*M.args(r))[4:]
    middle = ["K", "AE1", "T", "sp", "M", "AE1", "T", "DH", "AH0"]
    assert old_phns[rep[0][1]:rep[1][0]] == middle
    assert rep1[0] <= rep[0][0] and rep[1][1] <= rep1[1] and rep1 == [rep[0][0], rep[1][1]]
    # the two spans are the two words, in old and in new phones
    assert [old_phns[a:b] for a, b in rep] == [["S", "AE1", "T"], ["F", "AE1", "S", "T"]]
    assert [new_phns[a:b] for a, b in add] == [M.LEX["ZEBRA"], M.LEX["PLUM"]]
    new_wav, phns, ns, ne, old_b, new_b = plan
    assert phns == new_phns and len(ns) == len(ne) == len(phns) and len(old_b) == len(new_b) == 4
    # every kept phone keeps its label and its aligned duration, to one ulp of the shifted times
    kept_old = list(range(0, rep[0][0])) + list(range(rep[0][1], rep[1][0])) + list(range(rep[1][1], len(old_phns)))
    kept_new = list(range(0, add[0][0])) + list(range(add[0][1], add[1][0])) + list(range(add[1][1], len(phns)))
    assert len(kept_old) == len(kept_new) == len(old_phns) - 7
    for i, j in zip(kept_old, kept_new):
        assert phns[j] == old_phns[i]
        assert abs((ne[j] - ns[j]) - (me[i] - ms[i])) <= 2 * math.ulp(ne[j]), (i, j)
    assert ns[:rep[0][0]] == ms[:rep[0][0]] and all(a <= b for a, b in zip(ns, ne)) and all(b <= a for a, b in zip(ns[1:], ne))
    # the waveform: the original pieces sample for sample, zeros in the gaps, ceil(new_sum_k * fs) samples per gap
    factor = sedit.duration_adjust_factor([e - s for s, e in zip(ms, me)], dur(old_phns), old_phns)
    new_dur = [factor * d for d in dur(new_phns)]
    cuts = [(int(np.floor(ms[a] * fs)), int(np.ceil(me[b - 1] * fs))) for a, b in rep]
    gaps = []
    for (r0, r1), (a0, a1) in zip(rep, add):
        d = list(new_dur[a0:a1])
        if old_phns[r0] == new_phns[a0]:
            d[0] = me[r0] - ms[r0]
        gaps.append(int(np.ceil(sum(d) * fs)))
    assert all(g > 0 for g in gaps)
    org, pos, pieces = r.wav_org, 0, [(0, cuts[0][0]), (cuts[0][1], cuts[1][0]), (cuts[1][1], len(r.wav_org))]
    for k, (p0, p1) in enumerate(pieces):
        assert np.array_equal(new_wav[pos:pos + p1 - p0], org[p0:p1]) and (org[p0:p1] != 0).all()
        pos += p1 - p0
        if k < 2:
            assert not new_wav[pos:pos + gaps[k]].any()
            pos += gaps[k]
    assert pos == len(new_wav) and new_wav.dtype == org.dtype
    # frame spans: left to right, apart, the old ones around the old words
    assert old_b[0] < old_b[1] < old_b[2] < old_b[3] and new_b[0] < new_b[1] < new_b[2] < new_b[3]
    assert old_b[:2] == sedit.get_masked_mel_boundary(ms, me, fs, hop, rep[0])
    assert new_b[2:] == sedit.get_masked_mel_boundary(ns, ne, fs, hop, add[1])


def test_two_run_plan_masks_the_union_of_its_spans_in_both_collates(two_run):
    """plan_batch of the two-run request next to a single-span one: the flat span list goes to the collate, which pads the
    shorter list with zeros; masked_position (host path) is the union of the plan's new spans and nothing else, and the
    oracle's collate of the same input gives the same mask."""
    from a3t_amd import sedit
    from a3t_amd.collate import MLMCollateFn
    fx, waves, dur, r, spans, plan = two_run
    oc = O.tiny_config()
    one = M.request(fx, waves, M.SEVEN, max_spans=2, swap={2: "OWL"})
    plans, data = sedit.plan_batch([r, one], fx["fs"], fx["hop"], dur, _ids)
    assert plans[0].new_span_boundary == plan[5] and plans[0].old_span_boundary == plan[4] and len(plan[5]) == 4
    assert plans[0].new_spans == [plan[5][:2], plan[5][2:]] and plans[0].old_spans == [plan[4][:2], plan[4][2:]]
    assert len(plans[1].new_span_boundary) == 2 and plans[1].new_spans == [plans[1].new_span_boundary]
    assert np.array_equal(data[0][1]["span_boundary"], np.asarray(plan[5])) and np.array_equal(data[0][1]["speech"], plan[0])

    class HostFbank:
        fs, hop_length = oc.fs, oc.hop_length

        def __call__(self, wav, lengths):
            return O.logmel_fbank(wav, lengths, oc)

    coll = MLMCollateFn(HostFbank(), float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob, mean_phn_span=oc.mean_phn_span,
                        sega_emb=True)
    got = coll(data)[1]["masked_position"].numpy()
    ref = np.asarray(O.collate(data, oc)[1]["masked_position"])
    want = np.zeros_like(got)
    for b, p in enumerate(plans):
        for s, e in p.new_spans:
            want[b, s:e] = True
    assert want[0].sum() == sum(e - s for s, e in plans[0].new_spans) > 0
    assert np.array_equal(got, want) and np.array_equal(ref.reshape(want.shape), want)


# --------------------------------------------------------------------------------------------------------- planner rules
def test_max_spans_is_a_field_of_the_subclass_only():
    """EditRequest keeps its fields and their order; MultiSpanEditRequest adds max_spans (default 1) behind them, and
    dataclasses.replace carries it."""
    from dataclasses import fields
    from a3t_amd.sedit import EditRequest, MultiSpanEditRequest
    base = [f.name for f in fields(EditRequest)]
    assert base[-1] == "spembs" and "max_spans" not in base and not hasattr(EditRequest, "max_spans")
    assert [f.name for f in fields(MultiSpanEditRequest)] == base + ["max_spans"]
    r = MultiSpanEditRequest(None, [], {}, [], {}, "a", "b")
    assert r.max_spans == 1 and replace(replace(r, max_spans=3), old_str="c").max_spans == 3 and isinstance(r, EditRequest)


def test_max_spans_one_is_the_single_span_plan(two_run):
    from a3t_amd import sedit
    fx, waves, dur, r, _, _ = two_run
    one = sedit.get_phns_and_multi_spans(*M.args(r), max_spans=1)
    ref = sedit.get_phns_and_spans(*M.args(r))
    assert all(list(x) == list(y) for x, y in zip(one, ref)) and one[4] == ref[4] and isinstance(one[4][0], int)
    _same(sedit.prepare_features_multi(r.wav_org, fx["fs"], fx["hop"], *one, dur, r.new_str, **M.OPTS),
          sedit.prepare_features_with_duration(r.wav_org, fx["fs"], fx["hop"], *ref, dur, r.new_str, **M.OPTS))
    p1 = sedit.plan_batch([replace(r, max_spans=1)], fx["fs"], fx["hop"], dur, _ids)[0][0]
    p0 = sedit.plan_batch([sedit.EditRequest(*[getattr(r, k) for k in ("wav_org", "times2", "word2phns", "new_phns",
                                                                       "new_word2phns", "old_str", "new_str")], **M.OPTS)],
                          fx["fs"], fx["hop"], dur, _ids)[0][0]
    assert p1.new_span_boundary == p0.new_span_boundary and len(p1.new_span_boundary) == 2 and np.array_equal(p1.wav, p0.wav)


def test_three_runs_merge_the_pair_with_the_fewest_kept_phones_between():
    """BLUE [SAT] CAT sp [MAT] THE FAST [MAT] sp: four kept phones (CAT, sp) between the first two runs, six (THE, FAST)
    between the last two.  max_spans=3 keeps three spans, max_spans=2 merges the first pair -- the merged span replaces CAT
    and the `sp` with the new transcript's CAT --, max_spans=1 is the single-span plan."""
    from a3t_amd import sedit
    fx, waves, dur = M.fixture()
    r = M.request(fx, waves, M.SEVEN, swap={1: "ZEBRA", 3: "OWL", 6: "PLUM"})
    _, _, old, new3, rep3, add3 = sedit.get_phns_and_multi_spans(*M.args(r), max_spans=3)
    assert len(rep3) == 3 and [rep3[k + 1][0] - rep3[k][1] for k in range(2)] == [4, 6]
    assert [new3[a:b] for a, b in add3] == [M.LEX["ZEBRA"], M.LEX["OWL"], M.LEX["PLUM"]]
    assert sedit.get_phns_and_multi_spans(*M.args(r), max_spans=7)[4:] == (rep3, add3)
    _, _, _, new2, rep2, add2 = sedit.get_phns_and_multi_spans(*M.args(r), max_spans=2)
    assert rep2 == [[rep3[0][0], rep3[1][1]], rep3[2]]
    assert new2[add2[0][0]:add2[0][1]] == M.LEX["ZEBRA"] + ["K", "AE1", "T"] + M.LEX["OWL"]
    assert new2[add2[1][0]:add2[1][1]] == M.LEX["PLUM"] and new2[add2[0][1]:add2[1][0]] == old[rep2[0][1]:rep2[1][0]]
    # a tie goes to the leftmost pair: [A] DOG [A] RAN [CAT] sp MAT keeps three phones on both sides of the middle edit
    t = M.request(fx, waves, M.ONE_PHONE, swap={0: "ZEBRA", 2: "OWL", 4: "PLUM"})
    rep = sedit.get_phns_and_multi_spans(*M.args(t), max_spans=3)[4]
    assert rep == [[0, 1], [4, 5], [8, 11]] and [rep[k + 1][0] - rep[k][1] for k in range(2)] == [3, 3]
    assert sedit.get_phns_and_multi_spans(*M.args(t), max_spans=2)[4] == [[0, 5], [8, 11]]
    # and the pair on the right when fewer phones are kept there: BLUE [SAT] CAT sp MAT THE [FAST] MAT sp [+PLUM].  The merged
    # run is the words FAST MAT -> OWL MAT PLUM: the `sp` behind the last word lies between no two words of it and stays kept
    u = M.request(fx, waves, M.SEVEN, swap={1: "ZEBRA", 5: "OWL"}, insert={7: ["PLUM"]})
    rep = sedit.get_phns_and_multi_spans(*M.args(u), max_spans=3)[4]
    assert rep == [[3, 6], [15, 19], [23, 23]] and rep[1][0] - rep[0][1] > rep[2][0] - rep[1][1]
    _, _, old, new, rep, add = sedit.get_phns_and_multi_spans(*M.args(u), max_spans=2)
    assert rep == [[3, 6], [15, 22]] and old[22:] == ["sp"] == new[add[1][1]:]
    assert new[add[1][0]:add[1][1]] == M.LEX["OWL"] + ["M", "AE1", "T"] + M.LEX["PLUM"]


def test_a_deletion_next_to_a_replacement_merges_after_widening():
    """A DOG A RAN CAT sp MAT -> A ZEBRA A CAT MAT: the deletion of RAN is widened by one phone on each side, which is the whole
    one-phone word A between it and the replacement of DOG: the runs touch and become one span that is no longer widened."""
    from a3t_amd import sedit
    fx, waves, dur = M.fixture()
    r = M.request(fx, waves, M.ONE_PHONE, swap={1: "ZEBRA"}, drop=(3,))
    assert [o[0] for o in _runs(r)] == ["replace", "delete"]
    _, _, old, new, rep, add = sedit.get_phns_and_multi_spans(*M.args(r), max_spans=3)
    assert rep == [[1, 8]] and old[1:8] == ["D", "AO1", "G", "AH0", "R", "AE1", "N"]
    assert add == [[1, 7]] and new[1:7] == M.LEX["ZEBRA"] + ["AH0"] and new[7:] == old[8:]
    # a deletion that stays apart keeps its widening: one phone on each side, in both spans
    d = M.request(fx, waves, M.SEVEN, swap={1: "ZEBRA"}, drop=(5,))
    _, _, old, new, rep, add = sedit.get_phns_and_multi_spans(*M.args(d), max_spans=3)
    assert len(rep) == 2 and old[rep[1][0]:rep[1][1]] == ["AH0", "F", "AE1", "S", "T", "M"]
    assert new[add[1][0]:add[1][1]] == ["AH0", "M"]


def test_spans_whose_frames_touch_come_out_as_one():
    """Two phone spans with one kept phone of 1/256 s between them (less than a frame of 12.5 ms): the old frame spans touch,
    so one old and one new frame span come out; with 1/16 s between them two do.  (Times that binary floats hold exactly.)"""
    from a3t_amd import sedit
    fs, hop = 24000, 300
    for kept, want in ((1 / 256, 1), (1 / 16, 2)):
        durs = [0.125, 0.125, kept, 0.125, 0.125]
        ends = list(np.cumsum(durs))
        starts = [0.0] + ends[:-1]
        old = ["a", "b", "c", "d", "e"]
        new = ["a", "x", "c", "y", "e"]
        wav = np.arange(1, int(ends[-1] * fs) + 1, dtype=np.float32)
        out = sedit.prepare_features_multi(wav, fs, hop, starts, ends, old, new, [[1, 2], [3, 4]], [[1, 2], [3, 4]],
                                           lambda p: [0.125] * len(p), "a x c y e", duration_adjust=False)
        assert len(out[4]) == len(out[5]) == 2 * want, (kept, out[4], out[5])
        if want == 1:
            assert out[4] == [10, 30] and out[5] == [10, 30]
        else:
            assert out[4] == [10, 20, 25, 35] and out[5] == [10, 20, 25, 35]
        cut = sum(int(np.ceil(ends[b - 1] * fs)) - int(np.floor(starts[a] * fs)) for a, b in ([1, 2], [3, 4]))
        assert len(out[0]) == len(wav) - cut + 2 * 3000 and np.count_nonzero(out[0]) == len(wav) - cut


def test_an_insertion_has_an_empty_old_span():
    from a3t_amd import sedit
    fx, waves, dur = M.fixture()
    fs, hop = fx["fs"], fx["hop"]
    for at in (3, 7):       # in front of the first MAT (behind the `sp` that follows CAT), and behind the last entry
        r = M.request(fx, waves, M.SEVEN, swap={1: "ZEBRA"}, insert={at: ["PLUM"]})
        ms, me, old, new, rep, add = sedit.get_phns_and_multi_spans(*M.args(r), max_spans=2)
        p = rep[1][0]
        assert rep[1] == [p, p] and new[add[1][0]:add[1][1]] == M.LEX["PLUM"]
        if at == 3:
            assert old[p - 1] == "sp" and old[p:p + 3] == ["M", "AE1", "T"]
            f = int(np.floor(np.float32(fs) * np.float32(ms[p]) / hop))
        else:
            assert p == len(old)
            f = int(np.floor(np.float32(fs) * np.float32(me[-1]) / hop))
        wav, phns, ns, ne, old_b, new_b = sedit.prepare_features_multi(r.wav_org, fs, hop, ms, me, old, new, rep, add, dur, r.new_str,
                                                                       **M.OPTS)
        assert old_b[2:] == [f, f] and new_b[3] > new_b[2]
        # nothing is cut out for the insertion: the samples are all there, around the two gaps
        cut = int(np.ceil(me[rep[0][1] - 1] * fs)) - int(np.floor(ms[rep[0][0]] * fs))
        assert np.count_nonzero(wav) == len(r.wav_org) - cut


def test_append_and_mask_requests_ignore_max_spans():
    from a3t_amd import sedit
    fx, waves, dur = M.fixture()
    seen = set()
    for c in fx["cases"]:
        if c["kind"] in ("append", "mask", "mask_rec"):
            args = (c["times2"], c["word2phns"], c["new_phns"], c["new_word2phns"], c["old_str"], c["new_str"])
            a, b = sedit.get_phns_and_multi_spans(*args, max_spans=4), sedit.get_phns_and_spans(*args)
            assert all(list(x) == list(y) for x, y in zip(a, b))
            seen.add(c["kind"])
    assert seen == {"append", "mask", "mask_rec"}
    # an append that also changes an earlier word is still an append to the single-span planner only if old_str is a prefix
    r = M.request(fx, waves, M.SEVEN, insert={7: ["PLUM", "OWL"]})
    assert r.new_str.startswith(r.old_str)
    assert sedit.get_phns_and_multi_spans(*M.args(r), max_spans=3)[4] == sedit.get_phns_and_spans(*M.args(r))[4]
    with pytest.raises(ValueError, match="MASK"):
        sedit.prepare_features_multi(r.wav_org, 24000, 300, [0.0, 0.1, 0.2], [0.1, 0.2, 0.3], list("abc"), list("abc"),
                                     [[0, 1], [2, 3]], [[0, 1], [2, 3]], dur, "a [MASK] c")


# ------------------------------------------------------------------------------------------------------ windows and splice
def test_span_windows_separate_touching_and_clipped():
    from a3t_amd.vocoder import span_window, span_windows
    m, T = 14, 200
    apart, close = [[30, 40], [80, 95]], [[30, 40], [60, 70]]
    assert apart[1][0] - apart[0][1] > 2 * m and close[1][0] - close[0][1] <= 2 * m      # the premise of the two cases
    assert span_windows(apart, T, m) == [(16, 54), (66, 109)] == [span_window(s, e, T, m) for s, e in apart]
    assert span_windows(close, T, m) == [(16, 84)]
    assert span_windows([[30, 40], [68, 70]], T, m) == [(16, 84)]                        # windows that touch (54 == 54) merge
    assert span_windows([[30, 40], [69, 70]], T, m) == [(16, 54), (55, 84)]
    assert span_windows([[3, 10], [190, 200]], T, m) == [(0, 24), (176, 200)]            # clipped at both ends of the utterance
    assert span_windows([[0, 5], [10, 10], [150, 230]], T, m) == [(0, 24), (136, 200)]   # an empty span, and one beyond T
    assert span_windows([[40, 50]], 90, m) == [span_window(40, 50, 90, m)] and span_windows([], T, m) == []


def test_replace_waveform_multi_against_concatenation():
    from a3t_amd.sedit import replace_waveform, replace_waveform_multi
    hop = 4
    org = np.arange(100, dtype=np.float32)
    new = -np.arange(1, 121, dtype=np.float32)
    old_spans, new_spans = [[2, 5], [9, 9], [20, 25]], [[2, 7], [11, 14], [25, 27]]
    got = replace_waveform_multi(org, new, hop, old_spans, new_spans)
    want = np.concatenate([org[:8], new[8:28], org[20:36], new[44:56], org[36:80], new[100:108], org[100:]])
    assert np.array_equal(got, want) and got.dtype == np.float32
    for o, n in (([2, 5], [2, 7]), ([0, 0], [0, 3]), ([20, 25], [25, 30])):
        assert np.array_equal(replace_waveform_multi(org, new, hop, [o], [n]), replace_waveform(org, new, hop, o, n))
        assert np.array_equal(replace_waveform_multi(org, new, hop, o, n), replace_waveform(org, new, hop, o, n))
    with pytest.raises(ValueError):
        replace_waveform_multi(org, new, hop, old_spans, new_spans[:2])


def test_edit_batch_names_a_window_below_min_frames():
    """Two spans whose windows stay apart, the second one of three frames at the utterance's end with a margin of one: the
    editor refuses it by name before the vocoder is called."""
    from types import SimpleNamespace
    from a3t_amd.sedit import SpeechEditor

    class Voc:
        margin_frames, min_frames, calls = 1, 5, 0

        def inference(self, c, z=None, normalize_before=False, lengths=None):
            Voc.calls += 1
            return c[:, :, :1].repeat_interleave(2, dim=1)

    ed = SpeechEditor.__new__(SpeechEditor)
    ed.vocoder, ed.hop, ed.fs, ed._loaded = Voc(), 2, 24000, None
    mel = torch.zeros(1, 40, 4)
    plan = SimpleNamespace(old_span_boundary=[5, 12, 38, 40], new_span_boundary=[5, 12, 38, 40], old_spans=[[5, 12], [38, 40]],
                           new_spans=[[5, 12], [38, 40]])
    ed._decode_batch = lambda requests: ([plan], mel, None, [40])
    with pytest.raises(ValueError, match=r"window \[37, 40\).*min_frames = 5"):
        ed.edit_batch([SimpleNamespace(wav_org=np.ones(80, dtype=np.float32))], outputs=("orgin_replaced",))
    assert Voc.calls == 0


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_entries_are_declared_and_bound():
    from a3t_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "a3t_hip.h")).read()
    for name, nargs in (("a3t_splice_spans_multi", 13), ("a3t_gather_windows", 8)):
        m = re.search(rf"\bint {name}\(([^;]*)\);", hdr)
        assert m and name in _lib.EXPORTS and len(_lib._SIGS[name]) == nargs == len(m.group(1).split(",")), name
    assert callable(ops.splice_spans_multi) and callable(ops.gather_windows)
    src = open(os.path.join(ROOT, "a3t_amd", "csrc", "misc.hip")).read()
    assert 'extern "C" int a3t_splice_spans_multi(' in src and 'extern "C" int a3t_gather_windows(' in src


def test_edit_batch_window_rows_and_splice_on_a_recording_vocoder(monkeypatch):
    """edit_batch's own arithmetic around the vocoder, without a device: two requests, the first with two spans whose windows
    stay apart, the second with two spans whose windows merge -> three vocoder rows, gathered by ONE ops.gather_windows call
    (replaced here by the slicing it is specified as), z cut per window, every span spliced from its window; the result equals
    the whole-utterance call's.  The fake vocoder's sample t of a row is c[t // hop, 0] + z[t]."""
    from types import SimpleNamespace
    from a3t_amd import ops, sedit
    hop, flen, m = 3, [90, 50], 4
    tables = []

    def gather(src, table, dst):
        tables.append([tuple(int(x) for x in row) for row in table])
        dst.zero_()
        for r, (b, t0, n) in enumerate(table):
            dst[r, :n] = src[b, t0:t0 + n]

    monkeypatch.setattr(ops, "gather_windows", gather)

    class Voc:
        margin_frames, calls = m, []

        def inference(self, c, z=None, normalize_before=False, lengths=None):
            Voc.calls.append((tuple(c.shape), list(lengths)))
            y = c[:, :, :1].repeat_interleave(hop, dim=1).clone() + (0 if z is None else z)
            for b, n in enumerate(lengths):
                y[b, n * hop:] = 0
            return y

    ed = sedit.SpeechEditor.__new__(sedit.SpeechEditor)
    ed.vocoder, ed.hop, ed.fs, ed._loaded = Voc(), hop, 24000, None
    mel = torch.arange(2 * 96 * 2, dtype=torch.float32).reshape(2, 96, 2)
    spans = [([[10, 14], [40, 47]], [[10, 20], [46, 50]]), ([[5, 9], [12, 12]], [[5, 8], [11, 15]])]
    plans = [SimpleNamespace(old_span_boundary=[x for s in o for x in s], new_span_boundary=[x for s in n for x in s],
                             old_spans=o, new_spans=n) for o, n in spans]
    reqs = [SimpleNamespace(wav_org=-np.arange(1, 301, dtype=np.float32)), SimpleNamespace(wav_org=-np.arange(1, 151, dtype=np.float32))]
    ed._decode_batch = lambda requests: (plans, mel, None, list(flen))
    z = [np.random.RandomState(b).standard_normal(n * hop).astype(np.float32) for b, n in enumerate(flen)]
    full = ed.edit_batch(reqs, z=z)
    span = ed.edit_batch(reqs, outputs=("orgin_replaced",), z=z)
    assert Voc.calls == [((2, 96, 2), [90, 50]), ((3, 18, 2), [18, 12, 18])]
    assert tables == [[(0, 6, 18), (0, 42, 12), (1, 1, 18)]]
    for b, (f, s, r) in enumerate(zip(full, span, reqs)):
        (o0, o1), (p0, p1) = spans[b][0]
        (n0, n1), (m0, m1) = spans[b][1]
        pred = f["prediction"]
        assert np.array_equal(pred, mel[b, :flen[b], 0].numpy().repeat(hop) + z[b])
        want = np.concatenate([r.wav_org[:hop * o0], pred[hop * n0:hop * n1], r.wav_org[hop * o1:hop * p0], pred[hop * m0:hop * m1],
                               r.wav_org[hop * p1:]])
        assert np.array_equal(f["orgin_replaced"], want) and np.array_equal(s["orgin_replaced"], want) and "prediction" not in s
        assert s["new_spans"] == spans[b][1] and s["old_spans"] == spans[b][0] and s["new_span_boundary"] == plans[b].new_span_boundary
    # one window per request keeps the slice copies: no gather launch
    tables.clear()
    ed._decode_batch = lambda requests: (plans[1:], mel[1:], None, flen[1:])
    ed.edit_batch(reqs[1:], outputs=("orgin_replaced",))
    assert tables == [] and Voc.calls[-1] == ((1, 18, 2), [18])
