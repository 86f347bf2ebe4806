"""The vocoder's fp16-MFMA compute mode on the device (a3t_amd/csrc/pwg_fused_f16.hip, ParallelWaveGANGeneratorHIP(compute="f16"))
against the CPU restatement with the same rounding points (tests/pwg_f16_ref.py) and the fp32 oracle; the bit-for-bit properties
of the ragged and span-only paths in that mode.  Editor helpers follow tests/test_gpu_sedit_batch.py."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

import pwg_f16_ref as R
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
KINDS = ("replace", "mask", "append", "delete")


def _rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt(np.mean(a * a)))


# ------------------------------------------------------------------------------------------------------------- one block
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("dil", [1, 8, 512])
def test_one_block_against_the_restatement_of_one_block(dil, ragged):
    """a3t_pwg_block_f16 on random x, cu, skips (B = 2, Tw = 1500) against R.block with fp16 rounding.  What remains between the
    two is fp32 accumulation order, the fast exp and rare one-ulp flips of g: RMS(kernel - restatement) <= 0.1 x
    RMS(restatement - fp32 restatement), for x_out and for skips.  Rows behind W_b keep what they held."""
    from a3t_amd import ops
    from a3t_amd.vocoder import pack_pwg_block_f16, pwg_tile_list
    cfg, state = R.vocoder_state(seed=4)
    p = O.to_torch_state(state)
    pre = "conv_layers.3."
    B, Tw = 2, 1500
    W = (1500, 700) if ragged else (Tw, Tw)
    rs = np.random.RandomState(100 + dil)
    x = torch.from_numpy((rs.standard_normal((B, Tw, 64)) * 1.5).astype(np.float32))
    cu = torch.from_numpy((rs.standard_normal((B, Tw, 80)) * 2.0).astype(np.float32))
    sk = torch.from_numpy(rs.standard_normal((B, Tw, 64)).astype(np.float32))
    w0h, b0, w1h = pack_pwg_block_f16(p[pre + "conv.weight"], p[pre + "conv.bias"], p[pre + "conv1x1_aux.weight"],
                                      p[pre + "conv1x1_out.weight"])
    xd, skd = x.to(DEV).view(B * Tw, 64), sk.to(DEV).view(B * Tw, 64).clone()
    cu16 = torch.empty(B * Tw, 80, dtype=torch.float16, device=DEV)
    ops.cast_f16_sat(cu.to(DEV).view(B * Tw, 80), cu16)
    assert torch.equal(cu16.cpu().float().view(B, Tw, 80), R.rounder(torch.float16)(cu))
    xo = torch.full((B * Tw, 64), 777.0, device=DEV)
    tiles = torch.from_numpy(pwg_tile_list(W, 1)).to(DEV) if ragged else None
    ops.pwg_block_f16(xd, xo, cu16, w0h.to(DEV), b0.to(DEV), w1h.to(DEV), p[pre + "conv1x1_out.bias"].to(DEV), skd, tiles, B, Tw, dil)
    torch.cuda.synchronize()
    xo, sko = xo.cpu().view(B, Tw, 64), skd.cpu().view(B, Tw, 64)
    assert torch.equal(xd.cpu().view(B, Tw, 64), x)
    for b in range(B):
        n = W[b]
        xb, cb = x[b, :n].t()[None], cu[b, :n].t()[None]
        out = {}
        for name, dt in (("f16", torch.float16), ("f32", None)):
            rnd = R.rounder(dt)
            with torch.no_grad():
                xr, s = R.block(p, pre, xb, rnd(cb), dil, cfg, rnd)
            out[name] = (xr[0].t().numpy(), (sk[b, :n] + s[0].t()).numpy())
        for what, got, i in (("x_out", xo[b, :n].numpy(), 0), ("skips", sko[b, :n].numpy(), 1)):
            assert np.isfinite(got).all()
            res, rounding = _rms(got - out["f16"][i]), _rms(out["f16"][i] - out["f32"][i])
            print(f"block dil {dil} {'ragged' if ragged else 'dense'} row {b} ({n} samples) {what}: RMS(kernel - restatement) {res:.3e}, "
                  f"RMS(restatement - fp32 restatement) {rounding:.3e}, ratio {res / rounding:.4f}")
            assert res <= 0.1 * rounding, (what, b, res, rounding)
        assert (xo[b, n:] == 777.0).all() and torch.equal(sko[b, n:], sk[b, n:])


# ------------------------------------------------------------------------------------------------------- whole generator
def _table_case():
    cfg, state = R.vocoder_state(seed=4)
    c, z = R.table_inputs(40)
    return cfg, state, c, z


def test_generator_f16_against_the_fp32_oracle():
    """compute="f16" on the T = 40 input of the accuracy table against the CPU fp32 oracle: RMS and worst-element error each
    <= 2 x what the CPU restatement with fp16 rounding loses on the same input (the factor 2: the one-block residue accumulated
    over 30 layers), and below the bf16 restatement's."""
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    cfg, state, c, z = _table_case()
    p = O.to_torch_state(state)
    with torch.no_grad():
        ref = O.pwg_forward(p, c, z, cfg)
    r16 = R.errors(R.pwg_forward(p, c, z, cfg, torch.float16), ref)
    rb = R.errors(R.pwg_forward(p, c, z, cfg, torch.bfloat16), ref)
    gen = ParallelWaveGANGeneratorHIP(state, device=DEV, compute="f16")
    got = gen.inference(c.transpose(1, 2).contiguous(), z.transpose(1, 2).contiguous()).cpu()
    assert got.shape == (2, 40 * 300, 1) and torch.isfinite(got).all()
    e = R.errors(got.transpose(1, 2), ref)
    print(f"generator compute=f16 against the fp32 oracle: RMS {e[0]:.3e}, worst {e[1]:.3e}; CPU fp16 restatement {r16[0]:.3e}, "
          f"{r16[1]:.3e}; CPU bf16 restatement {rb[0]:.3e}, {rb[1]:.3e}")
    assert e[0] <= 2 * r16[0] and e[1] <= 2 * r16[1]
    assert e[0] < rb[0] and e[1] < rb[1]
    # single-utterance form
    one = gen.inference(c[1].t().contiguous(), z[1].t().contiguous()).cpu()
    assert torch.equal(one, got[1])


def test_ragged_rows_equal_single_runs_f16():
    """Rows of 61, 17, 3 and 40 frames in one padded batch, the padding of c and z filled with NaN, compute="f16": row b up to
    W_b is bit for bit what the row gives alone, the tail is exactly zero, nothing is NaN; lengths all equal to Tmax give the
    bits of lengths=None."""
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    cfg, state = R.vocoder_state(seed=41)
    lengths = (61, 17, 3, 40)
    B, Tmax, hop = len(lengths), max(lengths), 300
    rs = np.random.RandomState(3)
    c = (rs.standard_normal((B, Tmax, 80)) * 1.5 - 4.0).astype(np.float32)
    z = rs.standard_normal((B, Tmax * hop, 1)).astype(np.float32)
    cn, zn = c.copy(), z.copy()
    for b, n in enumerate(lengths):
        cn[b, n:] = np.nan
        zn[b, n * hop:] = np.nan
    gen = ParallelWaveGANGeneratorHIP(state, device=DEV, compute="f16")
    got = gen.inference(torch.from_numpy(cn), torch.from_numpy(zn), lengths=lengths)
    assert got.shape == (B, Tmax * hop, 1) and not torch.isnan(got).any()
    pv = O.to_torch_state(state)
    for b, n in enumerate(lengths):
        one = gen.inference(torch.from_numpy(c[b, :n]), torch.from_numpy(z[b, :n * hop]))
        d = float((got[b, :n * hop] - one).abs().max())
        print(f"f16 ragged row {b} ({n} frames) against the single run: max |diff| {d:.3e}")
        assert torch.equal(got[b, :n * hop], one), (b, d)
        assert not got[b, n * hop:].any()
        with torch.no_grad():
            ref = O.pwg_forward(pv, torch.from_numpy(c[b, :n]).t()[None], torch.from_numpy(z[b, :n * hop]).t()[None], cfg)
        rms, worst = R.errors(got[b, :n * hop].cpu().numpy(), ref.numpy())
        assert rms < 1e-2 and worst < 2e-2, (b, rms, worst)       # (sanity only: the accuracy checks are the two tests above)
    full = gen.inference(torch.from_numpy(c), torch.from_numpy(z))
    assert torch.equal(gen.inference(torch.from_numpy(c), torch.from_numpy(z), lengths=[Tmax] * B), full)


def test_two_calls_give_the_same_bits_and_leave_the_inputs_alone():
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    cfg, state, c, z = _table_case()
    gen = ParallelWaveGANGeneratorHIP(state, device=DEV, compute="f16")
    cd, zd = c.transpose(1, 2).contiguous().to(DEV), z.transpose(1, 2).contiguous().to(DEV)
    c0, z0 = cd.clone(), zd.clone()
    a = gen.inference(cd, zd)
    b = gen.inference(cd, zd)
    assert torch.equal(a, b)
    assert torch.equal(cd, c0) and torch.equal(zd, z0)
    ar = gen.inference(cd, zd, lengths=[40, 23])
    br = gen.inference(cd, zd, lengths=[40, 23])
    assert torch.equal(ar, br) and torch.equal(ar[0], a[0])
    assert torch.equal(cd, c0) and torch.equal(zd, z0)


def test_a_hot_conditioning_input_gives_a_finite_waveform():
    """c scaled until the upsampled conditioning exceeds 65504: the cast saturates, no infinity is made."""
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    cfg, state, c, z = _table_case()
    hot = c * 1e5
    stats = {}
    R.pwg_forward(O.to_torch_state(state), hot, z, cfg, torch.float16, stats)
    assert stats["max_cu"] > 65504.0
    gen = ParallelWaveGANGeneratorHIP(state, device=DEV, compute="f16")
    got = gen.inference(hot.transpose(1, 2).contiguous(), z.transpose(1, 2).contiguous())
    assert torch.isfinite(got).all()


def test_entry_point_refuses_aliasing_and_a_misaligned_tile_list():
    from a3t_amd import ops
    from a3t_amd._lib import A3TLibraryError
    from a3t_amd.vocoder import pack_pwg_block_f16, pwg_tile_list
    cfg, state = R.vocoder_state(seed=4)
    p = O.to_torch_state(state)
    pre = "conv_layers.0."
    w0h, b0, w1h = (t.to(DEV) for t in pack_pwg_block_f16(p[pre + "conv.weight"], p[pre + "conv.bias"], p[pre + "conv1x1_aux.weight"],
                                                          p[pre + "conv1x1_out.weight"]))
    b1 = p[pre + "conv1x1_out.bias"].to(DEV)
    B, Tw = 1, 300
    x, x2, sk = (torch.zeros(B * Tw, 64, device=DEV) for _ in range(3))
    cu16 = torch.zeros(B * Tw, 80, dtype=torch.float16, device=DEV)
    with pytest.raises(A3TLibraryError):
        ops.pwg_block_f16(x, x, cu16, w0h, b0, w1h, b1, sk, None, B, Tw, 1)
    tl = pwg_tile_list([Tw], 1)
    buf = torch.zeros(tl.size + 1, dtype=torch.int32, device=DEV)
    buf[1:] = torch.from_numpy(tl.reshape(-1)).to(DEV)
    with pytest.raises(A3TLibraryError):
        ops.pwg_block_f16(x, x2, cu16, w0h, b0, w1h, b1, sk, buf[1:].view(-1, 4), B, Tw, 1)
    with pytest.raises(ValueError):
        ops.pwg_block_f16(x, x2, cu16, w0h.float(), b0, w1h, b1, sk, None, B, Tw, 1)
    ops.pwg_block_f16(x, x2, cu16, w0h, b0, w1h, b1, sk, torch.from_numpy(tl).to(DEV), B, Tw, 1)      # the good call goes through
    torch.cuda.synchronize()
    assert torch.isfinite(x2).all()


def test_default_compute_is_f32_bit_for_bit():
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    cfg, state, c, z = _table_case()
    cd, zd = c.transpose(1, 2).contiguous(), z.transpose(1, 2).contiguous()
    a = ParallelWaveGANGeneratorHIP(state, device=DEV)
    b = ParallelWaveGANGeneratorHIP(state, device=DEV, compute="f32")
    assert a.compute == b.compute == "f32"
    assert torch.equal(a.inference(cd, zd), b.inference(cd, zd))
    assert torch.equal(a.inference(cd, zd, lengths=[40, 23]), b.inference(cd, zd, lengths=[40, 23]))
    assert not torch.equal(a.inference(cd, zd), ParallelWaveGANGeneratorHIP(state, device=DEV, compute="f16").inference(cd, zd))


# ------------------------------------------------------------------------------------------------------------ the editor
def _task_args(oc):
    enc = dict(input_layer="sega_mlm", cnn_module_kernel=oc.enc_kernel, attention_dim=oc.adim, attention_heads=oc.heads,
               linear_units=oc.ff, num_blocks=oc.enc_blocks, macaron_style=True, use_cnn_module=True,
               selfattention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos", positionwise_layer_type="conv1d",
               positionwise_conv_kernel_size=3)
    dec = dict(cnn_module_kernel=oc.dec_kernel, attention_dim=oc.adim, attention_heads=oc.heads, linear_units=oc.ff,
               num_blocks=oc.dec_blocks, selfattention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos")
    mc = dict(lsm_weight=0.1, mean_phn_span=8, mlm_prob=0.8, postnet_layers=oc.postnet_layers, postnet_filts=5,
              postnet_chans=oc.postnet_chans, dropout=False)
    return argparse.Namespace(token_list=[f"t{i}" for i in range(oc.vocab)], odim=80, input_size=80,
                              feats_extract="fbank", feats_extract_conf=dict(n_fft=2048, hop_length=300, win_length=1200,
                                                                             fs=24000, fmin=80, fmax=7600, n_mels=80),
                              normalize=None, normalize_conf={}, encoder="conformer", encoder_conf=enc,
                              decoder="conformer", decoder_conf=dec, model_conf=mc, init=None)


class _Vocoder:
    """The generator behind a recorder: `inference` passes through and records shapes and lengths."""

    def __init__(self, voc):
        self.voc, self.seen = voc, []

    @property
    def margin_frames(self):
        return self.voc.margin_frames

    def inference(self, c, z=None, normalize_before=False, lengths=None):
        self.seen.append((tuple(c.shape), None if lengths is None else list(lengths)))
        return self.voc.inference(c, z, normalize_before, lengths=lengths)


def _requests():
    from a3t_amd.sedit import EditRequest
    fx = json.load(open(os.path.join(G, "sedit.json")))
    waves = np.load(os.path.join(G, "sedit_wav.npz"))
    reqs = []
    for i, kind in enumerate(KINDS):
        empty = lambda c: c["plan"]["new_span_boundary"][0] == c["plan"]["new_span_boundary"][1]
        case = [c for c in fx["cases"] if c["kind"] == kind and (kind != "delete" or empty(c))][0]
        n = waves[case["wav"] + ".in"].shape[0]
        wav = (0.1 * np.random.RandomState(5 + i).standard_normal(n)).astype(np.float32)
        reqs.append(EditRequest(wav, case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"],
                                case["old_str"], case["new_str"], **case["opts"]))
    return reqs


def _editor(vocoder_compute):
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    from a3t_amd.sedit import SpeechEditor
    from a3t_amd.task import MLMTask
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden import fake_phone_duration
    oc = O.tiny_config()
    model = MLMTask.build_model(_task_args(oc), device=DEV, compute="f32")
    state = O.procedural_state(O.param_shapes(oc), 1)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    fe = LogMelFbank(fs=oc.fs, n_fft=oc.n_fft, win_length=oc.win_length, hop_length=oc.hop_length, n_mels=oc.n_mels,
                     fmin=oc.fmin, fmax=oc.fmax, device=DEV)
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob, mean_phn_span=oc.mean_phn_span,
                        sega_emb=True)
    cfg, vstate = R.vocoder_state(seed=4)
    voc = _Vocoder(ParallelWaveGANGeneratorHIP(vstate, device=DEV, compute=vocoder_compute))
    ids = lambda phns: np.array([2 + sum(map(ord, ph)) % (oc.vocab - 4) for ph in phns], dtype=np.int64)
    return SpeechEditor(model, coll, voc, ids, fake_phone_duration), oc


def test_edit_batch_span_only_equals_full_vocoding_f16():
    """edit_batch(outputs=("orgin_replaced",)) with an f16 vocoder: bit for bit the orgin_replaced of the full-vocoding call with
    the same noise, from fewer vocoded frames; and the f16 vocoder was really used (the result differs from the fp32 one)."""
    ed, oc = _editor("f16")
    reqs = _requests()
    flen = [x[1].shape[0] for x in ed.decode_batch(reqs)]
    z = [np.random.RandomState(20 + b).standard_normal((n * oc.hop_length, 1)).astype(np.float32) for b, n in enumerate(flen)]
    full = ed.edit_batch(reqs, z=z)
    ed.vocoder.seen.clear()
    span = ed.edit_batch(reqs, outputs=("orgin_replaced",), z=z)
    assert len(ed.vocoder.seen) == 1
    shape, lengths = ed.vocoder.seen[0]
    m = ed.vocoder.margin_frames
    bound = sum(f["new_span_boundary"][1] - f["new_span_boundary"][0] + 2 * m for f in full)
    print(f"f16 span-only: vocoded {sum(lengths)} frames (windows {lengths}) of {sum(flen)}; bound {bound}")
    assert sum(lengths) <= bound and sum(lengths) < sum(flen)
    for f, s in zip(full, span):
        assert "prediction" not in s and "prediction" in f
        d = float(np.abs(f["orgin_replaced"] - s["orgin_replaced"]).max()) if len(f["orgin_replaced"]) else 0.0
        print(f"f16 span-only against full vocoding: max |diff| {d:.3e}")
        assert np.array_equal(f["orgin_replaced"], s["orgin_replaced"])
    ed32, _ = _editor("f32")
    full32 = ed32.edit_batch(reqs, z=z)
    assert any(not np.array_equal(a["prediction"], b["prediction"]) for a, b in zip(full, full32))
    for a, b in zip(full, full32):
        if len(b["prediction"]):
            rms, worst = R.errors(a["prediction"], b["prediction"])
            print(f"f16 against f32 vocoder inside edit_batch: RMS {rms:.3e}, worst {worst:.3e}")
