"""Host side of dynamic evaluation (a3t_amd.sedit.dynamic_evaluation_batch) against tests/golden/dyneval.{npz,json}: what
the reference driver's own dynamic_evaluation built from synthetic stand-ins of its external programs (make_golden_dyneval.py).
No GPU: the collate runs on the oracle's CPU feature extractor (the integer tensors do not depend on the features)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import a3t_oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")


def _fixture():
    return json.load(open(os.path.join(G, "dyneval.json"))), np.load(os.path.join(G, "dyneval.npz"))


def _stand_ins(fx):
    phonemise = lambda line: (list(fx["phonemise"][line][0]), dict(fx["phonemise"][line][1]))
    ids = lambda phns: np.array([fx["token_ids"][ph] for ph in phns], dtype=np.int64)
    return phonemise, ids


def test_fixture_is_what_the_issue_asks_for():
    fx, z = _fixture()
    assert 5 <= len(fx["old_str"].split()) <= 7 and fx["n_entries"] == len(fx["old_str"].split()) - 1
    assert fx["steps"] == len(fx["losses"]) and all(b < a for a, b in zip(fx["losses"], fx["losses"][1:]))
    assert len(fx["param_names"]) == len(O.param_shapes(O.tiny_config())) - sum(
        1 for k in O.param_shapes(O.tiny_config()) if "running" in k or "num_batches" in k)
    for k in fx["param_names"]:
        assert z["grad." + k].shape == z["delta." + k].shape and z["grad." + k].size <= fx["n_sample"]
    assert fx["new_wav_len"] == fx["hop"] * (fx["mel_frames"] - fx["new_span_boundary"][0])


def test_batch_entries_match_the_reference():
    from a3t_amd.sedit import dynamic_evaluation_batch
    fx, z = _fixture()
    phonemise, ids = _stand_ins(fx)
    wav = z["wav"]
    batch = dynamic_evaluation_batch(wav, fx["times2"], fx["word2phns"], fx["old_str"], phonemise, ids, fx["fs"], fx["hop"])
    assert [u for u, _ in batch] == [str(i) for i in range(fx["n_entries"])]
    for i, (_, e) in enumerate(batch):
        assert set(e) == {"speech", "align_start", "align_end", "text", "span_boundary"}
        assert e["speech"] is wav                                   # the prompt itself: masked in place, nothing cut
        for k in ("align_start", "align_end", "text", "span_boundary"):
            ref = z[f"entry{i}.{k}"]
            assert e[k].dtype == ref.dtype and np.array_equal(e[k], ref), (i, k)
    # one entry per word but the last, in order: the spans move to the right and end before the last word's frames
    spans = [e["span_boundary"].tolist() for _, e in batch]
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    last_word_phones = len(list(fx["phonemise"][fx["new_str"]][1].values())[len(fx["old_str"].split()) - 1])
    spoken = [t for t in fx["times2"] if t[0] != "sp"]
    first_frame_of_last_word = int(np.floor(np.float32(fx["fs"]) * np.float32(spoken[-last_word_phones][1]) / np.float32(fx["hop"])))
    assert spans[-1][1] <= first_frame_of_last_word


def test_collated_integer_tensors_bit_for_bit():
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.sedit import dynamic_evaluation_batch
    fx, z = _fixture()
    phonemise, ids = _stand_ins(fx)
    oc = O.tiny_config()

    class CpuFbank:
        fs, hop_length = oc.fs, oc.hop_length

        def __call__(self, wav, lens):
            return O.logmel_fbank(wav, lens, oc)

    coll = MLMCollateFn(CpuFbank(), float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob,
                        mean_phn_span=oc.mean_phn_span, sega_emb=True)
    batch = dynamic_evaluation_batch(z["wav"], fx["times2"], fx["word2phns"], fx["old_str"], phonemise, ids, fx["fs"], fx["hop"])
    state = np.random.get_state()[1].copy()
    uids, out = coll(batch)
    assert np.array_equal(np.random.get_state()[1], state)          # span_boundary batches draw nothing
    names = [k[6:] for k in z.files if k.startswith("batch.")]
    assert set(names) == {"text", "masked_position", "speech_mask", "text_mask", "speech_segment_pos", "text_segment_pos",
                          "speech_lengths", "text_lengths"}
    for k in names:
        ref = z["batch." + k]
        got = out[k].numpy()
        assert got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(got, ref), k
    assert out["masked_position"].any(dim=1).all() and out["speech"].shape[:2] == out["masked_position"].shape


@pytest.mark.parametrize("old_str", ["hello", ""])
def test_one_word_prompt_is_an_error(old_str):
    from a3t_amd.sedit import dynamic_evaluation_batch
    with pytest.raises(ValueError, match="empty batch"):
        dynamic_evaluation_batch(np.zeros(2400, np.float32), [["HH", 0.0, 0.1]], {"0_HELLO": "HH"}, old_str,
                                 lambda s: (["[MASK]"], {"0_[MASK]": ["[MASK]"]}), lambda p: np.zeros(len(p), np.int64),
                                 24000, 300)


def test_sgd_step_is_exported_and_declared():
    from a3t_amd import _lib, ops
    assert "a3t_sgd_step" in _lib.EXPORTS and callable(ops.sgd_step)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "a3t_hip.h")).read()
    assert "int a3t_sgd_step(float* p, const float* g, int64_t n, float lr, float gscale, void* stream);" in hdr
