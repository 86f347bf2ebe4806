"""compute="bf16x3" through the engine and the model: fp32 storage and the fp32 schedule with the GEMMs on three bf16 MFMA
products (tests/test_gpu_gemm_x3.py holds the kernel).  Tiny config and procedural weights of tests/test_gpu_sedit_batch.py;
the oracle references of rows="alone" come from tests/mlm_rows_alone_ref.py, computed once."""
import collections

import numpy as np
import pytest
import torch

import mlm_rows_alone_ref as A
import test_gpu_sedit_batch as SB
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
# bf16x3 carries an operand to 2^-16 where bf16 carries it to 2^-8: its distance from fp32 is held to 2^-8 of bf16's, with a
# margin of 4 for the fp32 accumulation floor and the reordered sums
RATIO = 1.0 / 64


def _model(compute, train=False):
    from a3t_amd.task import MLMTask
    oc = O.tiny_config()
    model = MLMTask.build_model(SB._task_args(oc), device=DEV, compute=compute)
    state = O.procedural_state(O.param_shapes(oc), SB.MODEL_SEED)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.train(train)
    return model, oc


def _batch(oc):
    """B = 2, T_mel = 48, T_phn = 8 (T_mel and T_mel + T_phn multiples of 8: bf16 takes it unpadded), second row 40 / 6"""
    lens, tl = [48, 40], [8, 6]
    b = O.synthetic_batch(oc, B=2, T_mel=48, T_phn=8, seed=11, lengths=lens, text_lengths=tl)
    return {k: v.to(DEV) for k, v in b.items()}, lens


def _dist(x, ref, lens):
    """(RMS, worst element) of x - ref over the valid frames, float64"""
    d = torch.cat([(x[i, :n].double() - ref[i, :n].double()).reshape(-1) for i, n in enumerate(lens)])
    return float(d.pow(2).mean().sqrt()), float(d.abs().max())


def _forward(model, batch, need_grad=False):
    """the engine's forward with every GEMM's kernel name recorded: (out, Counter of kernel families)"""
    from a3t_amd import ops
    ops.PROFILE = rec = []
    try:
        with torch.no_grad():
            out = model._engine().forward(batch, need_grad=need_grad)
        torch.cuda.synchronize()
    finally:
        ops.PROFILE = None
    return out, collections.Counter(r[0].split("<")[0] for r in rec)


def test_forward_is_64_times_closer_to_fp32_than_bf16():
    """eval forward of one batch in "f32", "bf16" and "bf16x3": for `before` and `after`, RMS and worst element of bf16x3 - f32
    are at most 1/64 of those of bf16 - f32.  The bf16x3 model's GEMMs run on gemm_bf16x3_kernel (and on the fp32 kernel
    for what lies outside its alignment), the f32 model's on the fp32 kernel alone."""
    out, kern = {}, {}
    for compute in ("f32", "bf16", "bf16x3"):
        model, oc = _model(compute)
        batch, lens = _batch(oc)
        o, kern[compute] = _forward(model, batch)
        out[compute] = {k: o[k].float().clone() for k in ("before", "after")}
    print("GEMM kernels:", {k: dict(v) for k, v in kern.items()})
    assert set(kern["f32"]) == {"gemm_f32_kernel"}, kern["f32"]
    assert set(kern["bf16x3"]) <= {"gemm_bf16x3_kernel", "gemm_f32_kernel"} and kern["bf16x3"]["gemm_bf16x3_kernel"] > 0, kern["bf16x3"]
    for k in ("before", "after"):
        assert torch.isfinite(out["bf16x3"][k]).all()
        r16, w16 = _dist(out["bf16"][k], out["f32"][k], lens)
        r3, w3 = _dist(out["bf16x3"][k], out["f32"][k], lens)
        scale = max(1.0, float(out["f32"][k].abs().max()))
        print(f"{k}: bf16 - f32 rms {r16:.3e} worst {w16:.3e}; bf16x3 - f32 rms {r3:.3e} worst {w3:.3e}; "
              f"ratios {r3 / r16:.2e} / {w3 / w16:.2e} (bound {RATIO:.2e}); scale {scale:.2f}")
        assert r16 > 0 and r3 <= RATIO * r16, (k, r3, r16)
        assert w3 <= RATIO * w16, (k, w3, w16)


@pytest.fixture(scope="module")
def editor_x3():
    return SB._editor("bf16x3")


def test_rows_alone_against_the_oracle_alone(editor_x3):
    """the four fixture requests in one batch on a "bf16x3" model, rows="alone": per row the oracle's collate and forward of that
    request ALONE, atol = rtol = A.MEL_BOUND -- the fp32 test's own bound"""
    ed = editor_x3[0]
    assert ed.model.compute == "bf16x3"
    ref = A.oracle_rows_alone()
    reqs = SB._requests()
    p, mel, lens, flen = ed._decode_batch(reqs, rows="alone")
    assert lens.tolist() == flen == [int(r.shape[0]) for r in ref["rows"]]
    for i, (ob, nb) in enumerate(ref["plans"]):
        assert p[i].old_span_boundary == ob and p[i].new_span_boundary == nb
        L = flen[i]
        want = ref["rows"][i].numpy()
        print(f"row {i} ({L} frames, span {nb}): {A.of_scale(mel[i, :L].cpu().numpy(), want):.3e} of scale from the oracle alone")
        np.testing.assert_allclose(mel[i, :L].cpu().numpy(), want, atol=A.MEL_BOUND, rtol=A.MEL_BOUND)
        assert not mel[i, L:].any()
    got = ed.edit_batch(reqs, outputs=(), rows="alone")
    for i, g in enumerate(got):
        assert torch.equal(g["feat"], mel[i, :flen[i]])


def _short():
    model, oc = _model("bf16x3")
    p = O.to_torch_state(O.procedural_state(O.param_shapes(oc), SB.MODEL_SEED))
    b, sl, tl = A.short_batch(oc)
    return model, oc, p, b, sl, tl


def test_short_rows_against_the_oracle_alone():
    """rows (T_mel, T_phn) = (40, 3), (9, 8), (2, 1) in one padded batch: the row lengths are odd, the padded extents the GEMMs
    see are not.  Measured: all 28 GEMMs of this forward run on gemm_bf16x3_kernel and none falls back -- the three rows fit one
    chunk, so no B = 1 pass at exact odd lengths takes place here (a descriptor outside the alignment takes the fp32 kernel:
    tests/test_gpu_gemm_x3.py::test_routes; the assertion below admits both kernels and wants the new one at least once)"""
    from a3t_amd import ops
    model, oc, p, b, sl, tl = _short()
    ops.PROFILE = rec = []
    try:
        with torch.no_grad():
            mel, lens = model.inference_batch(**b, span_boundary=[[0, s] for s in sl], rows="alone")
        torch.cuda.synchronize()
    finally:
        ops.PROFILE = None
    kern = collections.Counter(r[0].split("<")[0] for r in rec)
    print("GEMM kernels:", dict(kern))
    assert set(kern) <= {"gemm_bf16x3_kernel", "gemm_f32_kernel"} and kern["gemm_bf16x3_kernel"] > 0, kern
    assert lens.tolist() == sl
    with torch.no_grad():
        for i, (s, t) in enumerate(zip(sl, tl)):
            want = O.model_forward(p, A.row_alone(b, i, s, t), oc, train_bn=False)[1][0].numpy()
            print(f"short row {i} ({s}, {t}): {A.of_scale(mel[i, :s].cpu().numpy(), want):.3e} of scale")
            np.testing.assert_allclose(mel[i, :s].cpu().numpy(), want, atol=A.MEL_BOUND, rtol=A.MEL_BOUND)
            assert not mel[i, s:].any()


def test_padding_content_changes_no_bit():
    """the protocol of tests/test_gpu_sedit_rows_alone.py on "bf16x3": frames behind sl_b and pad text ids set to large finite
    random values, the workspace filled with NaN between the two calls: no bit of the result changes"""
    model, oc, _, b, sl, tl = _short()
    spans = [[0, s] for s in sl]
    with torch.no_grad():
        mel0, _ = model.inference_batch(**b, span_boundary=spans, rows="alone")
        mel0 = mel0.clone()
        rs = np.random.RandomState(3)
        b1 = {k: v.clone() for k, v in b.items()}
        for i, (s, t) in enumerate(zip(sl, tl)):
            b1["speech"][i, s:] = torch.from_numpy((rs.standard_normal((40 - s, oc.idim)) * 50).astype(np.float32))
            b1["text"][i, t:] = torch.from_numpy(rs.randint(2, oc.vocab - 1, size=8 - t))
        for eng in model._eng.values():
            for t in eng.ws.bufs.values():
                if t.dtype == torch.float32:
                    t.fill_(float("nan"))
            eng.ws.pos_key = None
        mel1, _ = model.inference_batch(**b1, span_boundary=spans, rows="alone")
    assert torch.isfinite(mel1).all() and torch.equal(mel0, mel1)


def test_refusals_stay():
    """a "bf16" model still refuses rows="alone" and names `compute`; a misspelt mode is an error at every level, not fp32"""
    from a3t_amd.config import A3TConfig
    from a3t_amd.engine import MLMEngine
    from a3t_amd.params import ParamStore
    from a3t_amd.task import MLMTask
    model, oc = _model("bf16")
    b, sl, tl = A.short_batch(oc)
    with pytest.raises(ValueError, match="compute"):
        model.inference_batch(**b, span_boundary=[[0, s] for s in sl], rows="alone")
    ed = SB._editor("bf16")[0]
    with pytest.raises(ValueError, match="compute"):
        ed.edit_batch(SB._requests(), outputs=(), rows="alone")
    with pytest.raises(ValueError, match="bf16x2"):
        MLMTask.build_model(SB._task_args(oc), device=DEV, compute="bf16x2")
    c = A3TConfig(adim=oc.adim, heads=oc.heads, ff=oc.ff, enc_blocks=oc.enc_blocks, dec_blocks=oc.dec_blocks,
                  postnet_layers=oc.postnet_layers, postnet_chans=oc.postnet_chans, vocab=oc.vocab)
    with pytest.raises(ValueError, match="bf16x2"):
        MLMEngine(c, ParamStore(c, DEV), compute="bf16x2")
    # a refusal of ragged rows names the engine's own mode, not "f32"
    lens = (torch.tensor(sl, dtype=torch.int32, device=DEV), torch.tensor(tl, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="compute=bf16x3"):
        MLMEngine(c, ParamStore(c, DEV), compute="bf16x3", training=True).forward({k: v.to(DEV) for k, v in b.items()}, need_grad=False, lens=lens)


def test_one_training_step_runs():
    """forward + backward of one batch in "bf16x3", dropout off (the fp32 schedule with another GEMM flag): the loss is within
    RATIO of bf16's distance from the f32 engine's loss, and every gradient is finite and some are not 0.  Nothing tighter."""
    from a3t_amd.config import A3TConfig
    from a3t_amd.engine import MLMEngine
    from a3t_amd.params import ParamStore
    oc = O.tiny_config()
    c = A3TConfig(adim=oc.adim, heads=oc.heads, ff=oc.ff, enc_blocks=oc.enc_blocks, dec_blocks=oc.dec_blocks,
                  postnet_layers=oc.postnet_layers, postnet_chans=oc.postnet_chans, vocab=oc.vocab)
    store = ParamStore(c, DEV)
    state = O.procedural_state(O.param_shapes(oc), SB.MODEL_SEED)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    batch, _ = _batch(oc)
    loss, grads = {}, None
    for compute in ("f32", "bf16", "bf16x3"):
        eng = MLMEngine(c, store, compute=compute)
        loss[compute] = float(eng.forward(batch)["loss"])
        store.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        if compute != "bf16":
            g = {k: v.clone() for k, v in store.state_dict(grads=True).items()}
            if compute == "f32":
                grads = g
    d16, d3 = abs(loss["bf16"] - loss["f32"]), abs(loss["bf16x3"] - loss["f32"])
    print(f"loss f32 {loss['f32']:.7f} bf16 {loss['bf16']:.7f} bf16x3 {loss['bf16x3']:.7f}: |bf16x3 - f32| {d3:.3e}, |bf16 - f32| {d16:.3e}")
    assert d3 <= RATIO * d16, (d3, d16)
    for k, v in g.items():
        assert torch.isfinite(v).all(), k
    assert any(float(v.abs().max()) > 0 for v in g.values())
    # printed only: all gradients as one vector (tensors whose true gradient is 0, such as a bias in front of a BatchNorm, hold
    # rounding noise in both engines and say nothing one by one)
    a, b = torch.cat([v.reshape(-1).double() for v in g.values()]), torch.cat([grads[k].reshape(-1).double() for k in g])
    print(f"all gradients as one vector, bf16x3 against the f32 engine: relative L2 distance {float((a - b).norm() / b.norm()):.3e}")
