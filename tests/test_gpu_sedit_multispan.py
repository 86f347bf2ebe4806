"""Multi-span speech editing on the device: a3t_splice_spans_multi and a3t_gather_windows bit for bit, inference_batch with span
lists against the oracle (in the batch and rows="alone"), unchanged single-span calls, windowed against whole-utterance
vocoding for two vocoder classes, and the one device-to-host copy of edit_batch.  Tiny config, procedural weights and the editor
of tests/test_gpu_sedit_batch.py; requests from tests/sedit_multispan_ref.py."""
import functools

import numpy as np
import pytest
import torch

import mlm_rows_alone_ref as A
import sedit_multispan_ref as M
import test_gpu_sedit_batch as SB
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


@pytest.fixture(scope="module")
def editor():
    return SB._editor()


# ---------------------------------------------------------------------------------------------------------------- kernels
SPANS = np.array([[[0, 4], [10, 10], [20, 37]],         # starts at 0 | empty | ends exactly at the row's length 37
                  [[5, 60], [0, 0], [0, 0]],            # reaches beyond the row's length 30 (and beyond Tin); padded entries
                  [[3, 9], [9, 12], [30, 33]]],         # two adjacent ones -- and nspans = 0: none of them counts
                 dtype=np.int32)
NSPANS = (3, 1, 0)
ROW_LENS = (37, 30, 22)


@pytest.mark.parametrize("Tout", [37, 29, 45])
@pytest.mark.parametrize("C", [80, 6])
def test_splice_spans_multi_against_where(C, Tout):
    """B = 3, Tin = 37, S = 3, nspans (3, 1, 0), out and lens filled with NaN / garbage: bit for bit torch.where on a mask built
    from the spans; C = 80 takes the 16-byte path, C = 6 the scalar one.  Row 2 also carries its adjacent spans with nspans = 2,
    and with one span per row the result is a3t_splice_spans'."""
    from a3t_amd import ops
    B, Tin = 3, 37
    rs = np.random.RandomState(C + Tout)
    after, speech = rs.standard_normal((2, B, Tin, C)).astype(np.float32)
    mask = np.arange(Tin)[None] < np.asarray(ROW_LENS)[:, None]
    for nsp in (NSPANS, (3, 1, 2), (1, 1, 1)):
        out = torch.full((B, Tout, C), float("nan"), device=DEV)
        lens = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        ops.splice_spans_multi(_dev(after), _dev(speech), _dev(mask), _dev(SPANS), _dev(nsp, torch.int32), out, lens)
        inside = np.zeros((B, Tin), bool)
        for b in range(B):
            for s, e in SPANS[b, :nsp[b]]:
                inside[b, s:e] = True
        assert [int(x.sum()) for x in inside] == {NSPANS: [21, 32, 0], (3, 1, 2): [21, 32, 9], (1, 1, 1): [4, 32, 6]}[nsp]
        want = torch.where(torch.from_numpy(inside & mask)[..., None], torch.from_numpy(after), torch.from_numpy(speech))
        want = want * torch.from_numpy(mask)[..., None]
        ref = torch.zeros(B, Tout, C)
        n = min(Tin, Tout)
        ref[:, :n] = want[:, :n]
        assert lens.tolist() == list(ROW_LENS)
        assert not torch.isnan(out).any() and torch.equal(out.cpu(), ref), nsp
        if nsp == (1, 1, 1):
            one, l1 = torch.full_like(out, float("nan")), torch.full_like(lens, -7)
            ops.splice_spans(_dev(after), _dev(speech), _dev(mask), _dev(SPANS[:, 0]), one, l1)
            assert torch.equal(one, out) and torch.equal(l1, lens)


@pytest.mark.parametrize("C", [80, 6])
def test_gather_windows_against_slicing(C):
    """R = 4 windows of 2 source rows, lengths 1, 7, Wmax = 9 and 0, a NaN-filled destination: bit for bit the slices, zeros
    behind.  A table that leaves the source or the destination is refused before any launch."""
    from a3t_amd import ops
    B, T, Wmax = 2, 23, 9
    src = np.random.RandomState(C).standard_normal((B, T, C)).astype(np.float32)
    table = [(1, 22, 1), (0, 3, 7), (1, 0, 9), (0, 23, 0)]
    dst = torch.full((4, Wmax, C), float("nan"), device=DEV)
    ops.gather_windows(_dev(src), table, dst)
    ref = torch.zeros(4, Wmax, C)
    for r, (b, t0, n) in enumerate(table):
        ref[r, :n] = torch.from_numpy(src[b, t0:t0 + n])
    assert not torch.isnan(dst).any() and torch.equal(dst.cpu(), ref)
    for bad in ([(2, 0, 1)], [(0, 20, 4)], [(0, 0, 10)], [(-1, 0, 1)], [(0, -1, 2)]):
        with pytest.raises(ValueError):
            ops.gather_windows(_dev(src), bad, torch.empty(1, Wmax, C, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- infill
def _requests(spans=(2, 1, 3)):
    """Rows that plan as 2, 1 and 3 spans, on noise waveforms (a signal with a spectrum)."""
    fx, waves, _ = M.fixture()
    edits = {2: dict(swap={1: "ZEBRA", 5: "PLUM"}), 1: dict(swap={2: "OWL"}), 3: dict(swap={1: "ZEBRA", 3: "OWL", 6: "PLUM"})}
    index = {2: M.SEVEN, 1: M.LONG, 3: M.SEVEN}
    return [M.request(fx, waves, index[k], max_spans=3, wav=M.noise_wav(fx, waves, index[k], 11 + i), **edits[k])
            for i, k in enumerate(spans)]


@functools.lru_cache(maxsize=None)
def _oracle():
    """The oracle's chain for the three requests, computed once: the plans (the product's host planner, pinned by the host
    tests), ONE oracle collate and forward of the batch, and per request the collate and forward of that request alone; per row
    the mel spliced in numpy at the row's spans."""
    from a3t_amd import sedit
    oc = O.tiny_config()
    state = O.to_torch_state(O.procedural_state(O.param_shapes(oc), SB.MODEL_SEED))
    reqs = _requests()
    plans, data = sedit.plan_batch(reqs, oc.fs, oc.hop_length, A.fake_duration(), SB._ids(oc))

    def rows_of(batch, idx):
        with torch.no_grad():
            _, after = O.model_forward(state, batch, oc, train_bn=False)
        rows = []
        for i, b in enumerate(idx):
            L = int(batch["speech_mask"][i].sum())
            row = batch["speech"][i, :L].numpy().copy()
            for s, e in plans[b].new_spans:
                row[s:e] = after[i, s:e].numpy()
            rows.append(row)
        return rows

    batch = O.collate(data, oc)[1]
    return dict(plans=plans, data=data, batch=batch, rows=rows_of(batch, range(len(reqs))),
                alone=[rows_of(O.collate([d], oc)[1], [b])[0] for b, d in enumerate(data)])


@pytest.mark.parametrize("rows", ["batch", "alone"])
def test_inference_batch_with_span_lists_against_the_oracle(editor, rows):
    """Rows with 2, 1 and 3 spans in one batch, fp32.  rows="batch": per row the oracle's forward on the oracle's collate of the
    same batch, spliced at the row's spans, atol = rtol = 1e-3 (test_speech_editor_end_to_end_against_oracle).  rows="alone":
    against every request collated and run alone by the oracle, within the bound of test_edit_batch_rows_alone_against_edit
    (mlm_rows_alone_ref.MEL_BOUND).  Outside its spans a row IS the collated input mel, behind its length it is 0."""
    ed = editor[0]
    ref = _oracle()
    reqs = _requests()
    kw = {} if rows == "batch" else {"rows": rows}
    plans, mel, lens, flen = ed._decode_batch(reqs, **kw)
    assert [len(p.new_spans) for p in plans] == [2, 1, 3] == [len(p.old_spans) for p in plans]
    want = ref["rows"] if rows == "batch" else ref["alone"]
    assert lens.tolist() == flen == [int(r.shape[0]) for r in want] and len(set(flen)) > 1
    inp = ed.collate_fn(ref["data"], **kw)[1]["speech"]
    bound = 1e-3 if rows == "batch" else A.MEL_BOUND
    for i, p in enumerate(plans):
        assert p.new_span_boundary == ref["plans"][i].new_span_boundary
        L = flen[i]
        got = mel[i, :L].cpu().numpy()
        print(f"rows={rows!r}, row {i} ({L} frames, spans {p.new_spans}): max |diff| {float(np.abs(got - want[i]).max()):.3e}")
        np.testing.assert_allclose(got, want[i], atol=bound, rtol=bound)
        keep = np.ones(L, bool)
        for s, e in p.new_spans:
            keep[s:e] = False
            assert not np.array_equal(got[s:e], inp[i, s:e].cpu().numpy())
        assert np.array_equal(got[keep], inp[i, :L].cpu().numpy()[keep]) and not mel[i, L:].any()
    # the (B, S, 2) tensor form with counts gives the same bits
    feats = ed.collate_fn(ref["data"], **kw)[1]
    feats = {k: v for k, v in feats.items() if k not in ("span_boundary", "speech_lengths", "text_lengths")}
    sb = torch.zeros(3, 3, 2, dtype=torch.int32)
    for b, p in enumerate(plans):
        sb[b, :len(p.new_spans)] = torch.tensor(p.new_spans, dtype=torch.int32)
    with torch.no_grad():
        again, _ = ed.model.inference_batch(**feats, span_boundary=sb, span_counts=[2, 1, 3], **kw)
        assert torch.equal(again, mel)
        with pytest.raises(ValueError):
            ed.model.inference_batch(**feats, span_boundary=sb, **kw)


def _check_pieces(edited, wav_org, prediction, hop, old_spans, new_spans):
    """`edited` piece by piece: the recording outside the old spans, sample for sample, the vocoded frames of the new spans
    inside them (the kept audio is not re-timed: a kept piece has the OLD number of frames between two spans)."""
    pos, cut = 0, 0
    for (o0, o1), (n0, n1) in zip(old_spans, new_spans):
        keep = wav_org[cut:hop * o0]
        assert np.array_equal(edited[pos:pos + len(keep)], keep)
        pos += len(keep)
        assert np.array_equal(edited[pos:pos + hop * (n1 - n0)], prediction[hop * n0:hop * n1]) and n1 > n0
        pos += hop * (n1 - n0)
        cut = hop * o1
    assert np.array_equal(edited[pos:], wav_org[cut:]) and len(edited) == pos + len(wav_org[cut:])


# ------------------------------------------------------------------------------------------------------ unchanged calls
def test_single_run_request_with_max_spans_is_the_same_edit(editor):
    """edit(r, max_spans=2) on a request with one changed run is edit(r), bit for bit, key for key."""
    ed, oc = editor[0], editor[1]
    r = _requests((1,))[0]
    one = ed.edit(*SB._args(r), **M.OPTS)
    two = ed.edit(*SB._args(r), max_spans=2, **M.OPTS)
    assert set(one) == set(two) and one["new_span_boundary"] == two["new_span_boundary"] and len(one["new_span_boundary"]) == 2
    assert one["new_spans"] == [one["new_span_boundary"]] == two["new_spans"] and one["old_spans"] == two["old_spans"]
    assert torch.equal(one["feat"], two["feat"])
    for k in ("origin", "prediction", "orgin_replaced"):
        assert np.array_equal(one[k], two[k]), k


def test_edit_batch_of_one_two_span_request_equals_edit(editor):
    """edit_batch([r]) with a two-span r equals edit(r, max_spans=2) bit for bit in fp32, given the same noise; between the two
    spans orgin_replaced IS the recording."""
    ed, oc = editor[0], editor[1]
    hop = oc.hop_length
    r = _requests((2,))[0]
    one = ed.edit(*SB._args(r), max_spans=2, **M.OPTS)
    assert len(one["new_spans"]) == 2 and one["new_span_boundary"] == [x for s in one["new_spans"] for x in s]
    got = ed.edit_batch([r], z=[SB._Vocoder.noise(one["feat"].shape[0], hop)])[0]
    assert got["new_span_boundary"] == one["new_span_boundary"] and got["old_span_boundary"] == one["old_span_boundary"]
    assert got["new_spans"] == one["new_spans"] and got["old_spans"] == one["old_spans"]
    assert torch.equal(got["feat"], one["feat"])
    for k in ("origin", "prediction", "orgin_replaced"):
        assert np.array_equal(got[k], one[k]), (k, float(np.abs(got[k] - one[k]).max()))
    (o0, o1), (p0, p1) = one["old_spans"]
    assert p0 - o1 > 30
    _check_pieces(one["orgin_replaced"], r.wav_org, one["prediction"], hop, one["old_spans"], one["new_spans"])


# ------------------------------------------------------------------------------------------------------ windowed vocoding
def _window_requests():
    """Two two-span requests: DOG [ON] sp SAT QUIETLY MAT [TODAY] HOME (the kept run is far longer than two margins: the windows
    stay separate) and A [DOG] A [RAN] CAT sp MAT (one phone between the edits: the windows merge)."""
    fx, waves, _ = M.fixture()
    return [M.request(fx, waves, M.LONG, max_spans=2, wav=M.noise_wav(fx, waves, M.LONG, 31), swap={1: "ZEBRA", 5: "PLUM"}),
            M.request(fx, waves, M.ONE_PHONE, max_spans=2, wav=M.noise_wav(fx, waves, M.ONE_PHONE, 32), swap={1: "OWL", 3: "PLUM"})]


class _Recording:
    """A vocoder that records the lengths it is asked for."""

    def __init__(self, voc):
        self.voc, self.seen = voc, []
        self.margin_frames = voc.margin_frames
        if getattr(voc, "min_frames", None) is not None:
            self.min_frames = voc.min_frames

    def inference(self, c, z=None, normalize_before=False, lengths=None):
        self.seen.append((tuple(c.shape), list(lengths)))
        return self.voc.inference(c, z, normalize_before, lengths=lengths)


@pytest.mark.parametrize("family", ["pwg", "melgan"])
def test_windowed_vocoding_equals_whole_utterance_vocoding(family):
    """edit_batch(outputs=("orgin_replaced",)) on two two-span requests against the "orgin_replaced" of the call that vocodes
    whole utterances, bit for bit, with ParallelWaveGAN (given noise) and with multi-band MelGAN.  Request 0 keeps two windows
    and vocodes fewer frames than the hull of its spans, request 1's windows merge into one: three vocoder rows for two
    requests.  The audio between the spans is the recording, sample for sample."""
    from a3t_amd.vocoder import span_windows
    ed, oc, *_ = SB._editor()
    hop = oc.hop_length
    if family == "melgan":
        import test_gpu_melgan as MG
        ed.vocoder = _Recording(MG._gen("mb_v2_wn", True))
    else:
        ed.vocoder = _Recording(ed.vocoder.voc)
    m = ed.vocoder.margin_frames
    reqs = _window_requests()
    flen = [x[1].shape[0] for x in ed.decode_batch(reqs)]
    z = SB._batch_noise(flen, hop) if family == "pwg" else None
    full = ed.edit_batch(reqs, z=z)
    assert ed.vocoder.seen == [((2, max(flen), 80), flen)]
    ed.vocoder.seen.clear()
    span = ed.edit_batch(reqs, outputs=("orgin_replaced",), z=z)
    wins = [span_windows(f["new_spans"], flen[b], m) for b, f in enumerate(full)]
    # the premise: the first request's kept run is longer than two margins, the second's is not
    (a0, a1), (b0, b1) = full[0]["new_spans"]
    (c0, c1), (d0, d1) = full[1]["new_spans"]
    assert b0 - a1 > 2 * m and 0 < d0 - c1 <= 2 * m
    assert [len(w) for w in wins] == [2, 1]
    lengths = [w1 - w0 for w in wins for w0, w1 in w]
    assert ed.vocoder.seen == [((3, max(lengths), 80), lengths)]
    hull = b1 - a0
    print(f"{family}: windows {wins}, vocoded {lengths} frames; hull of request 0 {hull}, utterances {flen}")
    assert sum(lengths[:2]) < hull and lengths[2] == wins[1][0][1] - wins[1][0][0] >= d1 - c0
    for r, f, s in zip(reqs, full, span):
        assert "prediction" not in s and s["new_spans"] == f["new_spans"] and s["old_spans"] == f["old_spans"]
        assert np.array_equal(s["orgin_replaced"], f["orgin_replaced"]), float(np.abs(s["orgin_replaced"] - f["orgin_replaced"]).max())
        assert s["old_spans"][1][0] > s["old_spans"][0][1]
        _check_pieces(s["orgin_replaced"], r.wav_org, f["prediction"], hop, s["old_spans"], s["new_spans"])


def test_edit_batch_copies_to_the_host_once(editor):
    """Vocoding and splicing three windows of two requests add ONE device-to-host copy to what planning, collate and infill
    (_decode_batch) make on their own, as they do for one window per request."""
    ed = editor[0]
    reqs = _window_requests()
    orig, n = torch.Tensor.cpu, [0]

    def counting(self, *a, **k):
        n[0] += bool(self.is_cuda)
        return orig(self, *a, **k)

    ed.edit_batch(reqs, outputs=("orgin_replaced",))       # (warm)
    counts = []
    torch.Tensor.cpu = counting
    try:
        for call in (lambda: ed._decode_batch(reqs), lambda: ed.edit_batch(reqs, outputs=("orgin_replaced",)),
                     lambda: ed.edit_batch([reqs[0]], outputs=("orgin_replaced",)), lambda: ed._decode_batch([reqs[0]])):
            n[0] = 0
            call()
            counts.append(n[0])
    finally:
        torch.Tensor.cpu = orig
    assert counts[1] - counts[0] == 1 and counts[2] - counts[3] == 1, counts
