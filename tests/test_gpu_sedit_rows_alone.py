"""rows="alone" of the batched editor on the device: a row of a ragged batch against the SAME request collated and run alone
by the CPU oracle (the reference's driver is B = 1 throughout).  The two new kernels bit for bit, the ragged log-mel and the
collate against per-row calls, inference_batch / edit_batch against the oracle and against `edit`, short rows on two model
variants, the independence from the padding's content, chunking and the unchanged default.  Tiny config, procedural weights
and the four requests of tests/test_gpu_sedit_batch.py; references come from tests/mlm_rows_alone_ref.py, computed once."""
import numpy as np
import pytest
import torch

import mlm_rows_alone_ref as A
import mlm_variants_ref as V
import test_gpu_mlm_variants as MV
import test_gpu_sedit_batch as SB
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGMEL_BOUND = 2e-4       # the project's bound on device log-mel features (tests/test_gpu_features.py and the collate tests)


@pytest.fixture(scope="module")
def editor():
    return SB._editor()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _nan_workspace(model):
    """Every fp32 activation buffer of the model's engines holds NaN; the cached positional tables are rebuilt."""
    for eng in model._eng.values():
        for t in eng.ws.bufs.values():
            if t.dtype == torch.float32:
                t.fill_(float("nan"))
        eng.ws.pos_key = None


# ---------------------------------------------------------------------------------------------------------------- kernels
def test_reflect_pad_ragged_rows_are_the_rows_alone():
    """B = 3, N = 37, lengths (37, 9, 6), pad = 5 (the shortest legal row n = pad + 1 is there), the destination pre-filled
    with NaN and the samples behind a row's length NaN too: the row's extent is a3t_reflect_pad of the row alone, bit for
    bit, zeros behind it."""
    from a3t_amd import ops
    B, N, pad, lens = 3, 37, 5, (37, 9, 6)
    ld = (N + 2 * pad + 3) // 4 * 4
    x = np.random.RandomState(0).standard_normal((B, N)).astype(np.float32)
    xn = x.copy()
    for b, n in enumerate(lens):
        xn[b, n:] = np.nan
    out = torch.full((B, ld), float("nan"), device=DEV)
    ops.reflect_pad_ragged(_dev(xn), out, pad, _dev(lens, torch.int32), lens)
    assert not torch.isnan(out).any()
    for b, n in enumerate(lens):
        one = torch.full((1, n + 2 * pad), float("nan"), device=DEV)
        ops.reflect_pad(_dev(x[b:b + 1, :n]), one, pad)
        ref = np.pad(x[b, :n], pad, mode="reflect")
        assert np.array_equal(one[0].cpu().numpy(), ref)
        assert torch.equal(out[b, :n + 2 * pad], one[0]), b
        assert not out[b, n + 2 * pad:].any(), b


@pytest.mark.parametrize("shared", [False, True])
def test_concat_rows_ragged_packs_every_row(shared):
    """B = 3, Tm = 7, Tp = 5, D = 8, slens (7, 3, 1), tlens (2, 5, 1), destination pre-filled with NaN: bit for bit torch
    indexing, with a source per row and with source strides of 0 (one table behind every row)."""
    from a3t_amd import ops
    B, Tm, Tp, D, sl, tl = 3, 7, 5, 8, (7, 3, 1), (2, 5, 1)
    rs = np.random.RandomState(1)
    sp = _dev(rs.standard_normal((1 if shared else B, Tm, D)).astype(np.float32))
    tx = _dev(rs.standard_normal((1 if shared else B, Tp, D)).astype(np.float32))
    xs = torch.full((B, Tm + Tp, D), float("nan"), device=DEV)
    stride = dict(speech_bs=0, text_bs=0) if shared else {}
    ops.concat_rows_ragged(sp, tx, xs, _dev(sl, torch.int32), _dev(tl, torch.int32), B, Tm, Tp, D, **stride)
    ref = torch.zeros_like(xs)
    for b in range(B):
        k = 0 if shared else b
        ref[b, :sl[b]] = sp[k, :sl[b]]
        ref[b, sl[b]:sl[b] + tl[b]] = tx[k, :tl[b]]
    assert not torch.isnan(xs).any() and torch.equal(xs, ref)


# ---------------------------------------------------------------------------------------------------------------- collate
def test_logmel_rows_alone_against_per_row_calls(editor):
    """The four fixture waveforms in one padded call with rows="alone" against one call per waveform: the same frame counts,
    zeros behind a row's count, valid frames within the project's log-mel bound 2e-4 (no bit equality: a3t_gemm_plan may pick
    another kernel for another M).  rows="batch" differs from the rows alone by far more in a short row's last frames."""
    ed = editor[0]
    fe = ed.collate_fn.feats_extract
    waves = [d["speech"] for _, d in A.oracle_rows_alone()["data"]]
    slen = torch.tensor([len(w) for w in waves])
    x = torch.zeros(len(waves), int(slen.max()))
    for b, w in enumerate(waves):
        x[b, :len(w)] = torch.from_numpy(w)
    got, olens = fe(x, slen, rows="alone")
    old, _ = fe(x, slen)
    worst, worst_batch = 0.0, 0.0
    for b, w in enumerate(waves):
        one, n = fe(torch.from_numpy(w)[None], slen[b:b + 1])
        assert int(n[0]) == int(olens[b]) == one.shape[1]
        assert not got[b, int(n[0]):].any()
        worst = max(worst, float((got[b, :int(n[0])] - one[0]).abs().max()))
        worst_batch = max(worst_batch, float((old[b, :int(n[0])] - one[0]).abs().max()))
    print(f"log-mel, rows='alone' against per-row calls: max |diff| {worst:.3e} (rows='batch': {worst_batch:.3e})")
    assert worst <= LOGMEL_BOUND
    assert worst_batch > 0.1


@pytest.mark.parametrize("device_out", [False, True])
def test_collate_rows_alone_integer_outputs_are_the_single_request_collates(editor, device_out):
    """MLMCollateFn(rows="alone"), features through the host and with device_out: masks, segment ids and lengths bit-identical
    to the collate of every request alone, its mel within the log-mel bound of it."""
    from a3t_amd.collate import MLMCollateFn
    ed, oc = editor[0], editor[1]
    coll = MLMCollateFn(ed.collate_fn.feats_extract, float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob,
                        mean_phn_span=oc.mean_phn_span, sega_emb=True, device_out=device_out)
    data = SB._plan_data(ed, SB._requests())
    got = coll(data, rows="alone")[1]
    assert got["speech"].is_cuda == device_out
    for i, d in enumerate(data):
        one = coll([d])[1]
        for k, v in one.items():
            w = v.shape[-1] if v.dim() > 1 else None
            if k == "speech":
                n = v.shape[1]
                assert float((got[k][i, :n] - v[0]).abs().max()) <= LOGMEL_BOUND and not got[k][i, n:].any()
            elif w is None:
                assert torch.equal(got[k][i], v[0]), k
            else:
                assert torch.equal(got[k][i][..., :w], v[0]) and not got[k][i][..., w:].any(), (k, i)


# ---------------------------------------------------------------------------------------------------------------- infill
def test_inference_batch_rows_alone_against_the_oracle_alone(editor):
    """Four requests in one batch, fp32, rows="alone": per row the oracle's collate and forward of that request ALONE,
    spliced at its span, atol = rtol = 1e-3 (the bound of test_inference_batch_against_oracle).  Outside the span the row IS
    the alone-collated input mel, behind its length it is 0.  The same call with rows="batch" misses that reference by more
    than 0.1 on rows 0 and 1: the test sees the difference."""
    ed = editor[0]
    ref = A.oracle_rows_alone()
    reqs = SB._requests()
    p, mel, lens, flen = ed._decode_batch(reqs, rows="alone")
    assert lens.dtype == torch.int32 and lens.is_cuda
    assert lens.tolist() == flen == [int(r.shape[0]) for r in ref["rows"]]
    inp = ed.collate_fn(SB._plan_data(ed, reqs), rows="alone")[1]["speech"]
    _, old, _, _ = ed._decode_batch(reqs)
    for i, (ob, nb) in enumerate(ref["plans"]):
        assert p[i].old_span_boundary == ob and p[i].new_span_boundary == nb
        L, (s, e) = flen[i], nb
        want = ref["rows"][i].numpy()
        err = float(np.abs(mel[i, :L].cpu().numpy() - want).max())
        gap = float(np.abs(old[i, :L].cpu().numpy() - want)[s:e].max()) if e > s else 0.0
        print(f"row {i} ({L} frames, span [{s}, {e})): rows='alone' {err:.3e}, rows='batch' {gap:.3e} from the oracle alone")
        np.testing.assert_allclose(mel[i, :L].cpu().numpy(), want, atol=A.MEL_BOUND, rtol=A.MEL_BOUND)
        assert torch.equal(mel[i, :s].cpu(), inp[i, :s].cpu()) and torch.equal(mel[i, e:L].cpu(), inp[i, e:L].cpu())
        assert not mel[i, L:].any()
        if i in (0, 1):
            assert gap > A.SPAN_GAP, (i, gap)
    dec = ed.decode_batch(reqs, rows="alone")
    for i, (wav, feat, ob, nb) in enumerate(dec):
        assert torch.equal(feat, mel[i, :flen[i]]) and (ob, nb) == ref["plans"][i] and len(wav) == len(p[i].wav)


def test_edit_batch_rows_alone_against_edit(editor):
    """edit_batch(rows="alone") against ed.edit(r) per request: equal spans and lengths, feat within 1e-3, prediction and
    orgin_replaced with the same noise within the vocoder bound of test_edit_batch_against_oracle_chain."""
    ed, oc = editor[0], editor[1]
    reqs = SB._requests()
    ones = [ed.edit(*SB._args(r), **SB._opts(r)) for r in reqs]
    z = [SB._Vocoder.noise(o["feat"].shape[0], oc.hop_length) for o in ones]
    got = ed.edit_batch(reqs, z=z, rows="alone")
    for i, (g, o) in enumerate(zip(got, ones)):
        assert g["old_span_boundary"] == o["old_span_boundary"] and g["new_span_boundary"] == o["new_span_boundary"]
        assert g["feat"].shape == o["feat"].shape
        np.testing.assert_allclose(g["feat"].cpu().numpy(), o["feat"].cpu().numpy(), atol=A.MEL_BOUND, rtol=A.MEL_BOUND)
        atol = 2e-3 * max(1.0, float(np.abs(o["prediction"]).max()))
        for k in ("prediction", "orgin_replaced"):
            assert g[k].shape == o[k].shape, k
            print(f"request {i}, {k}: max |diff| to edit {float(np.abs(g[k] - o[k]).max()) if g[k].size else 0.0:.3e}")
            np.testing.assert_allclose(g[k], o[k], atol=atol, rtol=0)


def _short(case):
    """(model, oracle forward of one row alone, batch, slens, tlens) for the short rows on the default model or variant d."""
    c = O.tiny_config()
    if case == "default":
        from a3t_amd.task import MLMTask
        state = O.procedural_state(O.param_shapes(c), SB.MODEL_SEED)
        model = MLMTask.build_model(SB._task_args(c), device=DEV)
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
        p = O.to_torch_state(state)
        alone = lambda bb: O.model_forward(p, bb, c, train_bn=False)[1]
    else:
        model = MV._model(case)
        p = V.procedural(case)
        alone = lambda bb: V.variant_forward(p, bb, c, *V.CASES[case], train_bn=False)[1]
    model.eval()
    b, sl, tl = A.short_batch(c)
    return model, alone, b, sl, tl


@pytest.mark.parametrize("case", ["default", "d"])
def test_short_rows_against_the_oracle_alone(case):
    """Rows (T_mel, T_phn) = (40, 3), (9, 8), (2, 1) with given mels straight into inference_batch(rows="alone"), the whole row
    as the span: against the oracle's forward of each row alone.  (2, 1) is shorter than every depthwise kernel.  Also on the
    variant input_layer mlm + pre_speech_layer 1 + no_decoder."""
    model, alone, b, sl, tl = _short(case)
    with torch.no_grad():
        mel, lens = model.inference_batch(**b, span_boundary=[[0, s] for s in sl], rows="alone")
        assert lens.tolist() == sl
        for i, (s, t) in enumerate(zip(sl, tl)):
            want = alone(A.row_alone(b, i, s, t))[0].numpy()
            print(f"{case}: short row {i} ({s}, {t}): {A.of_scale(mel[i, :s].cpu().numpy(), want):.3e} of scale")
            np.testing.assert_allclose(mel[i, :s].cpu().numpy(), want, atol=A.MEL_BOUND, rtol=A.MEL_BOUND)
            assert not mel[i, s:].any()


def test_xvector_add_rows_alone_on_the_engine_and_training_engines_refuse():
    """MLMEngine.forward(lens=) itself, variant d with spk_embed_dim = 8: the projected x-vector reaches the speech and the text
    tokens of the packed rows (the restatement's x-vector add is the yardstick, as in test_gpu_mlm_variants).  An engine in
    training mode, or asked for gradients, refuses lens."""
    from a3t_amd.engine import MLMEngine
    from a3t_amd.params import ParamStore
    c = MV._cfg("d", spk_embed_dim=8)
    keys = dict(V.golden_keys("d"), **{"spk_proj.weight": (c.adim, 8), "spk_proj.bias": (c.adim,)})
    state = O.procedural_state(keys, seed=5)
    oc = O.tiny_config()
    b, sl, tl = A.short_batch(oc)
    b["spembs"] = torch.from_numpy(np.random.RandomState(2).standard_normal((3, 8)).astype(np.float32))
    store = ParamStore(c, DEV)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    lens = (_dev(sl, torch.int32), _dev(tl, torch.int32))
    bd = {k: v.to(DEV) for k, v in b.items()}
    out = MLMEngine(c, store, compute="f32", training=False).forward(bd, need_grad=False, lens=lens)
    p = O.to_torch_state(state)
    with torch.no_grad():
        for i, (s, t) in enumerate(zip(sl, tl)):
            want = V.variant_forward(p, A.row_alone(b, i, s, t), oc, *V.CASES["d"], train_bn=False)[1][0].numpy()
            np.testing.assert_allclose(out["after"][i, :s].cpu().numpy(), want, atol=A.MEL_BOUND, rtol=A.MEL_BOUND)
    with pytest.raises(ValueError, match="eval mode"):
        MLMEngine(c, store, compute="f32", training=True).forward(bd, need_grad=False, lens=lens)
    with pytest.raises(ValueError, match="forward only"):
        MLMEngine(c, store, compute="f32", training=False).forward(bd, need_grad=True, lens=lens)


@pytest.mark.parametrize("case", ["default", "d"])
def test_padding_content_changes_no_bit(case):
    """Frames behind sl_b and pad text ids set to large finite random values (finite: a masked probability 0 times a NaN value
    row is NaN in the probs @ V product, on the existing ragged path too) and the workspace filled with NaN between the two
    calls: no bit of the result changes."""
    model, _, b, sl, tl = _short(case)
    c = O.tiny_config()
    spans = [[0, s] for s in sl]
    with torch.no_grad():
        mel0, _ = model.inference_batch(**b, span_boundary=spans, rows="alone")
        mel0 = mel0.clone()
        rs = np.random.RandomState(3)
        b1 = {k: v.clone() for k, v in b.items()}
        for i, (s, t) in enumerate(zip(sl, tl)):
            b1["speech"][i, s:] = torch.from_numpy((rs.standard_normal((40 - s, c.idim)) * 50).astype(np.float32))
            b1["text"][i, t:] = torch.from_numpy(rs.randint(2, c.vocab - 1, size=8 - t))
        _nan_workspace(model)
        mel1, _ = model.inference_batch(**b1, span_boundary=spans, rows="alone")
    assert torch.isfinite(mel1).all() and torch.equal(mel0, mel1)


# ------------------------------------------------------------------------------------------------- chunking and the default
def test_chunking_stays_within_the_bound_and_the_default_is_unchanged(editor):
    """A max_score_elems that cuts the four requests into three chunks, one of them a single row (the B = 1 path at the row's
    exact lengths), against the one-chunk call: within atol = rtol = 1e-3 of it, the same lengths.  With the masks on the
    device the one-chunk call asks for no lengths on the host.  edit_batch(reqs) and edit_batch(reqs, rows="batch") are
    bit-identical."""
    from a3t_amd.engine import score_chunks
    ed = editor[0]
    reqs = SB._requests()
    feats = ed.collate_fn(SB._plan_data(ed, reqs), rows="alone")[1]
    feats = {k: v for k, v in feats.items() if k not in ("span_boundary", "speech_lengths", "text_lengths")}
    spans = [list(pl[1]) for pl in A.oracle_rows_alone()["plans"]]
    H = ed.model.cfg.heads
    n = [int(feats["speech_mask"][i].sum() + feats["text_mask"][i].sum()) for i in range(len(reqs))]
    order = sorted(n)
    cap = 2 * H * order[1] ** 2           # the two shortest rows together, then the third alone, then the longest alone
    chunks = score_chunks(n, H, cap)
    assert [len(ch) for ch in chunks] == [2, 1, 1], chunks
    with torch.no_grad():
        one, l1 = ed.model.inference_batch(**feats, span_boundary=spans, rows="alone")
        cut, l3 = ed.model.inference_batch(**feats, span_boundary=spans, rows="alone", max_score_elems=cap)
        ondev, l2 = ed.model.inference_batch(**{k: v.to(DEV) for k, v in feats.items()}, span_boundary=spans, rows="alone")
    assert l1.tolist() == l3.tolist() == l2.tolist()
    print(f"three chunks {chunks} against one: max |diff| {float((one - cut).abs().max()):.3e}")
    np.testing.assert_allclose(cut.cpu().numpy(), one.cpu().numpy(), atol=A.MEL_BOUND, rtol=A.MEL_BOUND)
    np.testing.assert_allclose(ondev.cpu().numpy(), one.cpu().numpy(), atol=A.MEL_BOUND, rtol=A.MEL_BOUND)
    a = ed.edit_batch(reqs, outputs=())
    b = ed.edit_batch(reqs, outputs=(), rows="batch")
    for x, y in zip(a, b):
        assert torch.equal(x["feat"], y["feat"])
