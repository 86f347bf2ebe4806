"""rows="alone" of the batched editor, host side: the fixture guard (a row in the batch really differs from the row alone),
the packed-row rule on the oracle's own blocks, the refusals and the C ABI of the two new entry points."""
import os
import re

import numpy as np
import pytest
import torch

import mlm_rows_alone_ref as A
import mlm_variants_ref as V
from oracle import a3t_oracle as O


# ---------------------------------------------------------------- the fixture guard
def test_fixture_rows_in_the_batch_differ_from_the_rows_alone():
    """The oracle's collate and model_forward on the four fixture requests as ONE batch against each request alone, seed 1:
    rows 0 and 1 miss by >= 0.1 inside their spans (100 x the device test's bound 1e-3), the longest row agrees within 1e-5.
    This passes with and without rows="alone": it is what keeps the device test meaningful."""
    ref = A.oracle_rows_alone()
    oc, plans = ref["oc"], ref["plans"]
    b = O.collate(ref["data"], oc)[1]
    with torch.no_grad():
        _, after = O.model_forward(ref["state"], b, oc, train_bn=False)
    frames = [int(x["speech"].shape[1]) for x in ref["batches"]]
    longest = int(np.argmax(frames))
    assert longest == 2 and b["text_mask"][longest].all()          # the append request is the longest row on both sides
    for i, (_, (s, e)) in enumerate(plans):
        gap = float((after[i, s:e] - ref["after"][i][s:e]).abs().max()) if e > s else 0.0
        mel = float((b["speech"][i, :frames[i]] - ref["batches"][i]["speech"][0]).abs().max())
        print(f"row {i}: {frames[i]} frames, span [{s}, {e}): batch against alone {gap:.3e} in the span, collated mel {mel:.3e}")
        if i in (0, 1):
            assert gap >= A.SPAN_GAP, (i, gap)
        if i == longest:
            assert gap <= 1e-5 and mel <= 1e-5, (i, gap, mel)


# ---------------------------------------------------------------- the packed-row rule
def test_packed_rows_equal_the_rows_alone_default_model():
    """packed_forward on the alone-collated batch of the four requests: every row equals the oracle's forward of the request
    alone within 1e-5 of scale, over the whole row (not only the span)."""
    ref = A.oracle_rows_alone()
    oc = ref["oc"]
    b = A.alone_collated_batch(ref)
    sl = [int(x["speech"].shape[1]) for x in ref["batches"]]
    tl = [int(x["text"].shape[1]) for x in ref["batches"]]
    with torch.no_grad():
        _, after = A.packed_forward(ref["state"], b, oc, sl, tl)
    for i, n in enumerate(sl):
        err = A.of_scale(after[i, :n].numpy(), ref["after"][i].numpy())
        print(f"packed row {i} ({n} frames, {tl[i]} phones) against the row alone: {err:.3e} of scale")
        assert err <= A.RULE_BOUND, (i, err)


@pytest.mark.parametrize("case", ["default", "d"])
def test_packed_short_rows_equal_the_rows_alone(case):
    """Rows (T_mel, T_phn) = (40, 3), (9, 8), (2, 1), the padding of the mels and the text ids filled with finite random
    values: the default model, and the variant d (input_layer mlm, pre_speech_layer 1, no_decoder)."""
    c = O.tiny_config()
    if case == "default":
        p = O.to_torch_state(O.procedural_state(O.param_shapes(c), 1))
        seg, pre, dec = True, 0, True
        alone = lambda bb: O.model_forward(p, bb, c, train_bn=False)[1]
    else:
        p = V.procedural(case)
        seg, pre, dec = V.CASES[case]
        alone = lambda bb: V.variant_forward(p, bb, c, seg, pre, dec, train_bn=False)[1]
    b, sl, tl = A.short_batch(c)
    rs = np.random.RandomState(3)
    for i, (s, t) in enumerate(zip(sl, tl)):
        b["speech"][i, s:] = torch.from_numpy((rs.standard_normal((40 - s, c.idim)) * 50).astype(np.float32))
        b["text"][i, t:] = torch.from_numpy(rs.randint(2, c.vocab - 1, size=8 - t))
    with torch.no_grad():
        _, after = A.packed_forward(p, b, c, sl, tl, seg, pre, dec)
        for i, (s, t) in enumerate(zip(sl, tl)):
            want = alone(A.row_alone(b, i, s, t))[0]
            err = A.of_scale(after[i, :s].numpy(), want.numpy())
            print(f"{case}: packed short row {i} ({s}, {t}) against the row alone: {err:.3e} of scale")
            assert err <= A.RULE_BOUND, (case, i, err)


# ---------------------------------------------------------------- the collate with a host extractor
def test_collate_rows_alone_with_a_host_extractor_calls_it_once_per_row():
    """An extractor without a device (here the oracle's logmel_fbank) is called once per row with the row's own samples: the
    batch's mels are the single-request collates' bit for bit, zeros behind, and the integer outputs are theirs too.  The
    default call still hands it the padded batch once."""
    from a3t_amd.collate import MLMCollateFn
    ref = A.oracle_rows_alone()
    oc = ref["oc"]
    calls = []

    class HostFbank:
        fs, hop_length = oc.fs, oc.hop_length

        def __call__(self, wav, lengths):
            calls.append(tuple(wav.shape))
            return O.logmel_fbank(wav, lengths, oc)

    coll = MLMCollateFn(HostFbank(), float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob,
                        mean_phn_span=oc.mean_phn_span, sega_emb=True)
    got = coll(ref["data"], rows="alone")[1]
    assert calls == [(1, len(d["speech"])) for _, d in ref["data"]]
    want = A.alone_collated_batch(ref)
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    calls.clear()
    coll(ref["data"])
    assert calls == [(len(ref["data"]), max(len(d["speech"]) for _, d in ref["data"]))]


# ---------------------------------------------------------------- refusals
class _Fe:
    """What the editor reads of a feature extractor; no test here extracts features."""
    fs, hop_length = O.tiny_config().fs, O.tiny_config().hop_length


def _cpu_editor(compute="f32", collate=None):
    import test_gpu_sedit_batch as SB
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.sedit import SpeechEditor
    from a3t_amd.task import MLMTask
    oc = O.tiny_config()
    model = MLMTask.build_model(SB._task_args(oc), device="cpu", compute=compute)
    model.eval()
    coll = collate or MLMCollateFn(_Fe(), sega_emb=True)
    return SpeechEditor(model, coll, None, SB._ids(oc), A.fake_duration()), SB._requests()


def test_unknown_rows_value_is_refused():
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    ed, reqs = _cpu_editor()
    for call in (lambda: ed.edit_batch(reqs, rows="each"), lambda: ed.decode_batch(reqs, rows="each"),
                 lambda: MLMCollateFn(None)([], rows="each"),
                 lambda: LogMelFbank(device="cpu")(torch.zeros(1, 4000), rows="each"),
                 lambda: ed.model.inference_batch(*[torch.zeros(1, 1)] * 7, span_boundary=[[0, 0]], rows="each")):
        with pytest.raises(ValueError, match="rows"):
            call()


def test_bf16_model_refuses_rows_alone_and_names_compute():
    ed, reqs = _cpu_editor("bf16")
    with pytest.raises(ValueError, match="compute"):
        ed.edit_batch(reqs, rows="alone")
    with pytest.raises(ValueError, match="compute"):
        ed.model.inference_batch(*[torch.zeros(1, 1)] * 7, span_boundary=[[0, 0]], rows="alone")


def test_collate_without_rows_is_refused_and_named():
    class PlainCollate:
        feats_extract = _Fe()

        def __call__(self, data):
            raise AssertionError("must not be called")
    ed, reqs = _cpu_editor(collate=PlainCollate())
    with pytest.raises(ValueError, match="PlainCollate"):
        ed.edit_batch(reqs, rows="alone")
    with pytest.raises(ValueError, match="PlainCollate"):
        ed.decode_batch(reqs, rows="alone")


def test_dynamic_eval_stays_refused_in_batches():
    from dataclasses import replace
    ed, reqs = _cpu_editor()
    with pytest.raises(ValueError, match="ONE prompt"):
        ed.edit_batch([reqs[0], replace(reqs[1], dynamic_eval=(5e-5, 1))], rows="alone")


def test_reflect_pad_ragged_refuses_a_row_not_longer_than_the_pad():
    """The host check of ops.reflect_pad_ragged names the row, as torch.stft refuses a waveform that reflection cannot pad;
    nothing is launched (CPU tensors)."""
    from a3t_amd import ops
    x, out = torch.zeros(3, 37), torch.zeros(3, 48)
    with pytest.raises(ValueError, match="row 2"):
        ops.reflect_pad_ragged(x, out, 5, torch.tensor([37, 9, 5], dtype=torch.int32), [37, 9, 5])
    with pytest.raises(ValueError, match="row 1"):
        ops.reflect_pad_ragged(x, out, 5, torch.tensor([37, 38, 6], dtype=torch.int32), [37, 38, 6])


def test_score_chunks_is_the_duration_models_chunking():
    from a3t_amd.engine import score_chunks
    assert score_chunks([5, 3, 9, 3], 2, 2 * 2 * 25) == [[1, 3], [0], [2]]
    assert score_chunks([5, 3, 9, 3], 2, 1 << 24) == [[1, 3, 0, 2]]
    assert score_chunks([40], 2, 1) == [[0]]


# ---------------------------------------------------------------- C ABI
def test_new_exports_are_declared_with_matching_signatures():
    from a3t_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "a3t_hip.h")).read(), flags=re.S)
    want = {"a3t_reflect_pad_ragged": [True, True, True, False, False, False, False, True],
            "a3t_concat_rows_ragged": [True, True, True, True, True, False, False, False, False, False, False, True]}
    for name, ptrs in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert name in _lib.EXPORTS and len(args) == len(_lib._SIGS[name]) == len(ptrs), (name, args)
        assert [("*" in a) for a in args] == ptrs
    declared = set(re.findall(r"\b(a3t_\w+)\s*\(", txt))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in want)
