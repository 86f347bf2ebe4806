"""Host half of batched speech editing: plan_batch against the per-request plan, the oracle and the reference driver's own
outputs (tests/golden/sedit.json), the vocoder's margin / window arithmetic, and the claim span-window vocoding rests on,
checked on the oracle's generator.  No GPU."""
import json
import os
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

from oracle import a3t_oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")
KINDS = ("replace", "mask", "append", "delete")


def _fixture():
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden import fake_phone_duration
    return json.load(open(os.path.join(G, "sedit.json"))), np.load(os.path.join(G, "sedit_wav.npz")), fake_phone_duration


def _ids(phns):
    return np.array([2 + sum(map(ord, ph)) % 36 for ph in phns], dtype=np.int64)


def _requests(fx, waves, kinds=KINDS):
    from a3t_amd.sedit import EditRequest
    reqs, cases = [], []
    for kind in kinds:
        case = [c for c in fx["cases"] if c["kind"] == kind][0]
        reqs.append(EditRequest(waves[case["wav"] + ".in"], case["times2"], case["word2phns"], case["new_phns"],
                                case["new_word2phns"], case["old_str"], case["new_str"], **case["opts"]))
        cases.append(case)
    return reqs, cases


def test_plan_batch_equals_per_request_plan_and_oracle():
    from a3t_amd import sedit
    fx, waves, dur = _fixture()
    fs, hop = fx["fs"], fx["hop"]
    reqs, cases = _requests(fx, waves)
    calls = []

    def counting(phns):
        calls.append(tuple(phns))
        return dur(phns)

    plans, data = sedit.plan_batch(reqs, fs, hop, counting, _ids)
    assert len(plans) == len(data) == len(reqs) and [u for u, _ in data] == ["0", "1", "2", "3"]
    assert len(calls) == len(set(calls))                # the duration model ran once per distinct phone list
    for r, c, p, (_, d) in zip(reqs, cases, plans, data):
        args = (r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str)
        ms, me, op, nph, rep, add = sedit.get_phns_and_spans(*args)
        one = sedit.prepare_features_with_duration(r.wav_org, fs, hop, ms, me, op, nph, rep, add, dur, r.new_str, **c["opts"])
        ref = O.sedit_plan_edit(r.wav_org, fs, hop, *O.sedit_phone_spans(*args), dur, r.new_str, **c["opts"])
        for other in (one, ref):
            assert np.array_equal(p.wav, np.asarray(other[0])) and p.wav.dtype == np.float32
            assert list(p.phns) == list(other[1])
            assert list(p.align_start) == list(other[2]) and list(p.align_end) == list(other[3])
            assert list(p.old_span_boundary) == [int(x) for x in other[4]]
            assert list(p.new_span_boundary) == [int(x) for x in other[5]]
        assert p.old_span_boundary == c["plan"]["old_span_boundary"] and p.new_span_boundary == c["plan"]["new_span_boundary"]
        assert np.array_equal(p.wav, waves[c["wav"] + ".out"])
        # the collate input: one span_boundary per item
        assert set(d) == {"speech", "align_start", "align_end", "text", "span_boundary"}
        assert np.array_equal(d["span_boundary"], np.asarray(p.new_span_boundary)) and np.array_equal(d["speech"], p.wav)
        assert np.array_equal(d["text"], _ids(p.phns)) and len(d["align_start"]) == len(d["align_end"]) == len(p.phns)
    spans = [tuple(p.new_span_boundary) for p in plans]
    assert len(set(spans)) == len(spans)


def test_plan_batch_refuses_dynamic_eval_and_empty_batches():
    from a3t_amd import sedit
    fx, waves, dur = _fixture()
    reqs, _ = _requests(fx, waves, KINDS[:2])
    with pytest.raises(ValueError, match="ONE prompt"):
        sedit.plan_batch([reqs[0], replace(reqs[1], dynamic_eval=(5e-5, 1))], fx["fs"], fx["hop"], dur, _ids)
    with pytest.raises(ValueError):
        sedit.plan_batch([], fx["fs"], fx["hop"], dur, _ids)


def test_margin_frames_follows_the_formula():
    from a3t_amd.vocoder import pwg_margin_frames
    assert pwg_margin_frames() == 14                                    # v1 at hop 300: R = 3069, U = 395, ceil(3464 / 300) + 2
    assert pwg_margin_frames(30, 3, 3, (4, 5, 3, 5), 2) == 14
    # 10 layers in 1 stack, scales (4, 4, 4, 4): R = 1023, U = 256 + 64 + 16 + 4 = 340, hop 256: ceil(1363 / 256) + 2 = 8
    assert pwg_margin_frames(10, 1, 3, (4, 4, 4, 4), 2) == 8
    # 8 layers in 2 stacks, kernel 5, scales (8, 8), no context: R = 2 * 15 * 2 = 60, U = 64 + 8 = 72, hop 64: ceil(132 / 64) = 3
    assert pwg_margin_frames(8, 2, 5, (8, 8), 0) == 3


def test_span_window_arithmetic():
    from a3t_amd.vocoder import span_window
    m = 14
    assert span_window(40, 50, 90, m) == (26, 64)
    assert span_window(3, 10, 90, m) == (0, 24)             # clipped at the start
    assert span_window(80, 90, 90, m) == (66, 90)           # clipped at the end
    assert span_window(5, 85, 90, m) == (0, 90)             # clipped at both ends
    assert span_window(0, 90, 90, m) == (0, 90)             # the span is the whole utterance
    assert span_window(40, 40, 90, m) == (26, 54)           # an empty span still has its surroundings
    assert span_window(90, 90, 90, m) == (76, 90)           # pure append behind the last frame
    assert span_window(0, 0, 0, m) == (0, 0)


def test_ragged_tile_list_covers_exactly_the_valid_samples():
    from a3t_amd.vocoder import pwg_tile_list
    lengths, hop = (61, 0, 3, 40), 300
    tl = pwg_tile_list(lengths, hop)
    assert tl.dtype == np.int32 and tl.shape[1] == 4
    want = [(b, t0, n * hop, 0) for b, n in enumerate(lengths) for t0 in range(0, n * hop, 256)]
    assert [tuple(int(v) for v in r) for r in tl] == want
    assert pwg_tile_list([0, 0], hop).shape == (0, 4)


@pytest.mark.parametrize("span", [(0, 12), (38, 55), (77, 90)])
def test_window_reproduces_the_full_run_inside_the_span_on_the_oracle(span):
    """The claim span-window vocoding rests on: the oracle's generator on span +- margin_frames, clipped to the utterance and
    fed the same slice of the noise, gives inside the span what it gives on the whole utterance (bound of test_pwg)."""
    from a3t_amd.vocoder import pwg_margin_frames, span_window
    cfg = O.PWGConfig()
    state = O.procedural_state(O.pwg_param_shapes(cfg), seed=4)
    for k in state:
        if "up_layers" in k:
            state[k] = np.abs(state[k]) / np.abs(state[k]).sum()
    p = O.to_torch_state(state)
    T, hop = 90, 300
    rs = np.random.RandomState(2)
    c = torch.from_numpy((rs.standard_normal((1, 80, T)) * 1.5 - 4.0).astype(np.float32))
    z = torch.from_numpy(rs.standard_normal((1, 1, T * hop)).astype(np.float32))
    m = pwg_margin_frames(cfg.layers, cfg.stacks, cfg.kernel_size, cfg.upsample_scales, cfg.aux_context_window)
    assert m == 14
    n0, n1 = span
    w0, w1 = span_window(n0, n1, T, m)
    with torch.no_grad():
        full = O.pwg_forward(p, c, z, cfg)[0, 0].numpy()
        win = O.pwg_forward(p, c[:, :, w0:w1], z[:, :, w0 * hop:w1 * hop], cfg)[0, 0].numpy()
    got, ref = win[(n0 - w0) * hop:(n1 - w0) * hop], full[n0 * hop:n1 * hop]
    print(f"span {span} window {(w0, w1)}: max |diff| {np.abs(got - ref).max():.3e} at scale {np.abs(ref).max():.3f}")
    np.testing.assert_allclose(got, ref, atol=1e-5, rtol=1e-4)
