"""Dynamic evaluation and prompt-based TTS on the device: the SGD kernel, eval-mode gradients of the engine and of the
model surface against the CPU oracle, the adaptation trajectory against the reference's own run
(tests/golden/dyneval.{npz,json}, make_golden_dyneval.py) and the SpeechEditor driver."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"

# fp32 bounds of test_e2e_tiny_against_reference_golden (train mode), used for eval mode unchanged
LOSS_RTOL = 1e-4
GRAD_ATOL, GRAD_RTOL = 5e-4, 5e-3       # atol = GRAD_ATOL * max(1, max|ref|)
# the project's stated bf16 bounds (tests/test_gpu_parity_r2.py)
BF16_LOSS_RTOL, BF16_COS = 1e-2, 0.99


def _fixture():
    return json.load(open(os.path.join(G, "dyneval.json"))), np.load(os.path.join(G, "dyneval.npz"))


def _engine(oc, seed, compute="f32", training=False):
    from test_gpu_e2e import _engine as make
    return make(oc, seed, compute=compute, training=training)


def _to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _oracle_eval_grads(oc, seed, batch):
    p = O.to_torch_state(O.procedural_state(O.param_shapes(oc), seed), requires_grad=True)
    loss, before, after = O.forward_loss(p, batch, oc, train_bn=False)
    loss.backward()
    grads = {k: t.grad.numpy() for k, t in p.items() if t.grad is not None}
    return float(loss), before.detach().numpy(), after.detach().numpy(), grads


def _buffers(store):
    return {k: v.clone() for k, v in store.state_dict().items() if "running" in k or "num_batches" in k}


def _assert_grads_fp32(grads, ref, what=""):
    worst = (0.0, "")
    for k, r in ref.items():
        got = grads[k].cpu().numpy()
        atol = GRAD_ATOL * max(1.0, float(np.abs(r).max()))
        err = float((np.abs(got - r) / (atol + GRAD_RTOL * np.abs(r))).max())
        worst = max(worst, (err, k))
        np.testing.assert_allclose(got, r, atol=atol, rtol=GRAD_RTOL, err_msg=f"{what}{k}")
    return worst


# ------------------------------------------------------------------ 2. the SGD kernel
def test_sgd_step_kernel_bit_exact_with_guards():
    """a3t_sgd_step against p - (lr * gscale) * g computed by torch in fp32 on the same device, the step rounded to fp32 once
    as the kernel does.  Bit-equal: the library is built without FMA contraction and torch's multiply and subtract are two
    kernels' worth of roundings too (no ulp of slack was needed).  Sizes cover the scalar-only case, the n % 4 tail, a buffer
    at a 4-byte offset (no 16-byte alignment: scalar loop throughout) and the tiny model's parameter count; guard words on
    either side must stay as they were."""
    from a3t_amd import ops
    oc = O.tiny_config()
    n_model = _engine(oc, 1)[1].total
    gen = torch.Generator(device="cpu").manual_seed(3)
    for n in (1, 3, 4, 1023, 4096 + 5, n_model):
        for lr, gscale, shift in ((1e-2, 1.0, 0), (5e-5, 1.0, 0), (0.3, 0.125, 0), (1e-2, 1.0, 1), (7e-3, 3.0, 3)):
            guard = 8
            pbuf = torch.randn(n + 2 * guard + shift, generator=gen).to(DEV)
            gbuf = torch.randn(n + 2 * guard + shift, generator=gen).to(DEV)
            p, g = pbuf[guard + shift:guard + shift + n], gbuf[guard + shift:guard + shift + n]
            before_p, before_g = pbuf.clone(), gbuf.clone()
            step = torch.tensor(np.float32(lr) * np.float32(gscale), dtype=torch.float32, device=DEV)
            want = before_p[guard + shift:guard + shift + n] - step * g
            ops.sgd_step(p, g, lr, gscale)
            torch.cuda.synchronize()
            assert torch.equal(p, want), (n, lr, gscale, shift, float((p - want).abs().max()))
            assert torch.equal(pbuf[:guard + shift], before_p[:guard + shift]) and torch.equal(pbuf[guard + shift + n:], before_p[guard + shift + n:])
            assert torch.equal(gbuf, before_g)
    with pytest.raises(ValueError):
        ops.sgd_step(torch.zeros(4, device=DEV), torch.zeros(5, device=DEV), 0.1)


# ------------------------------------------------------------------ 3. eval-mode gradients of the engine
def test_eval_mode_gradients_fp32_against_oracle():
    """MLMEngine(training=False): forward(need_grad=True) + backward() against oracle.forward_loss(train_bn=False) under
    autograd -- loss 1e-4 relative, every gradient tensor within atol = 5e-4 * max(1, max|ref|), rtol = 5e-3; running
    statistics and num_batches_tracked untouched; and a forward-only pass gives the same bits before and after."""
    oc = O.tiny_config()
    batch = O.synthetic_batch(oc, B=2, T_mel=48, T_phn=8, seed=11, lengths=[48, 37], text_lengths=[8, 6])
    ref_loss, ref_b, ref_a, ref = _oracle_eval_grads(oc, 1, batch)
    assert len(ref) == 93                                    # every parameter tensor of tiny_config gets a gradient
    eng, store = _engine(oc, 1)
    bufs = _buffers(store)
    b = _to_dev(batch)
    fo = {k: v.clone() for k, v in eng.forward(b, need_grad=False).items()}
    out = eng.forward(b, need_grad=True)
    loss = float(out["loss"])
    print(f"eval fp32 loss {loss!r} oracle {ref_loss!r} rel {abs(loss - ref_loss) / abs(ref_loss):.2e}")
    assert abs(loss - ref_loss) < LOSS_RTOL * abs(ref_loss)
    np.testing.assert_allclose(out["before"].cpu().numpy(), ref_b, atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out["after"].cpu().numpy(), ref_a, atol=2e-4, rtol=1e-4)
    store.zero_grad()
    eng.backward()
    torch.cuda.synchronize()
    worst = _assert_grads_fp32(store.state_dict(grads=True), ref)
    print(f"eval fp32 gradients: worst error {worst[0]:.3f} of the bound ({worst[1]})")
    for k, v in _buffers(store).items():
        assert torch.equal(v, bufs[k]), k
    again = eng.forward(b, need_grad=False)
    assert eng._need_grad is False and eng._fused_train_now is False
    for k in ("loss", "before", "after"):
        assert torch.equal(again[k], fo[k]), k
    # a second gradient pass accumulates the same gradient again (flat buffer semantics of a training step)
    g1 = store.grad.clone()
    eng.forward(b, need_grad=True)
    eng.backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(store.grad.cpu().numpy(), 2 * g1.cpu().numpy(), rtol=1e-4, atol=1e-5 * float(g1.abs().max()))


@pytest.mark.parametrize("fused_train", [False, True])
def test_eval_mode_gradients_bf16_against_oracle(fused_train, monkeypatch):
    """The bf16 engine in eval mode against the oracle's fp32 gradients: loss 1e-2 relative, cosine >= 0.99 for every
    gradient tensor (full vectors).  `linear_k.bias` has an analytically zero gradient (softmax shift invariance), so a
    cosine does not exist for it; tests/test_gpu_parity_r2.py leaves it out for the same reason and so does this test.
    (A bias in front of BatchNorm is NOT zero here: in eval mode the layer subtracts the running mean, not the batch's.)
    fused_train: the batch is big enough (64 attention workgroups) for both fused attention kernels, the forward-only one
    and, with gradients, the one that saves the probabilities -- here without dropout; otherwise the materialised path."""
    from a3t_amd.espnet_model import ESPnetMLMEncAsDecoderModel
    monkeypatch.delenv("A3T_FUSED_ATTN", raising=False)
    monkeypatch.delenv("A3T_FUSED_ATTN_TRAIN", raising=False)
    oc = O.A3TConfig(enc_blocks=1, dec_blocks=1, postnet_layers=2, postnet_chans=16)
    B = 32 if fused_train else 2
    batch = O.synthetic_batch(oc, B=B, T_mel=50, T_phn=9, seed=13, lengths=[50, 41] + [50] * (B - 2),
                              text_lengths=[9, 7] + [9] * (B - 2))
    pb = ESPnetMLMEncAsDecoderModel._pad_to_dma_granule(dict(batch))
    ref_loss, _, _, ref = _oracle_eval_grads(oc, 2, pb)
    eng, store = _engine(oc, 2, compute="bf16")
    bufs = _buffers(store)
    b = _to_dev(pb)
    fo = {k: v.clone() for k, v in eng.forward(b, need_grad=False).items()}
    assert eng._fused_now == fused_train
    out = eng.forward(b, need_grad=True)
    assert eng._fused_train_now == fused_train and not eng._fused_now
    loss = float(out["loss"])
    print(f"eval bf16 loss {loss!r} oracle {ref_loss!r} rel {abs(loss - ref_loss) / abs(ref_loss):.2e}")
    assert abs(loss - ref_loss) < BF16_LOSS_RTOL * abs(ref_loss)
    store.zero_grad()
    eng.backward()
    torch.cuda.synchronize()
    grads = store.state_dict(grads=True)
    bad, worst = [], (1.0, "")
    for k, r in ref.items():
        got = grads[k].cpu().numpy().astype(np.float64).reshape(-1)
        r = r.astype(np.float64).reshape(-1)
        if k.endswith("linear_k.bias"):
            print(f"{k}: max |gradient| {float(np.abs(got).max()):.2e} (oracle {float(np.abs(r).max()):.2e}; analytically 0)")
            continue
        cos = float((got * r).sum() / (np.linalg.norm(got) * np.linalg.norm(r) + 1e-300))
        worst = min(worst, (cos, k))
        if cos < BF16_COS:
            bad.append((k, round(cos, 4)))
    print(f"eval bf16 gradients (fused_train={fused_train}): worst cosine {worst[0]:.4f} ({worst[1]})")
    assert not bad, bad
    for k, v in _buffers(store).items():
        assert torch.equal(v, bufs[k]), k
    again = eng.forward(b, need_grad=False)
    assert eng._fused_now == fused_train and not eng._fused_train_now     # still the forward-only attention path
    for k in ("loss", "before", "after"):
        assert torch.equal(again[k], fo[k]), k


# ------------------------------------------------------------------ 4. the model surface
def _model(oc, seed, compute="f32"):
    from a3t_amd.task import MLMTask
    from test_gpu_e2e import _task_args
    model = MLMTask.build_model(_task_args(oc), device=DEV, compute=compute)
    state = O.procedural_state(O.param_shapes(oc), seed)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    return model, state


def test_model_eval_mode_loss_backward():
    """model.eval(); loss, _, _ = model(**batch); loss.backward() fills p.grad with the eval-mode gradients (the reference
    model's contract, which its dynamic_evaluation relies on); under torch.no_grad() the pass stays forward-only."""
    oc = O.tiny_config()
    batch = O.synthetic_batch(oc, B=2, T_mel=48, T_phn=8, seed=11, lengths=[48, 37], text_lengths=[8, 6])
    ref_loss, _, _, ref = _oracle_eval_grads(oc, 1, batch)
    model, _ = _model(oc, 1)
    bufs = _buffers(model.store)
    with torch.no_grad():
        l0, _, _ = model(**batch)
    assert l0.grad_fn is None and not l0.requires_grad
    loss, stats, weight = model(**batch)
    assert loss.grad_fn is not None and torch.equal(loss.detach(), l0)
    assert abs(float(loss) - ref_loss) < LOSS_RTOL * abs(ref_loss)
    model.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    for name, p in model._params.items():
        assert p.grad is not None and torch.equal(p.grad, model.store.g[name]), name
    _assert_grads_fp32(model.store.state_dict(grads=True), ref, "model ")
    for k, v in _buffers(model.store).items():
        assert torch.equal(v, bufs[k]), k
    # an optimiser over model.parameters() now does what the reference's dynamic evaluation does
    flat0 = model.store.flat.clone()
    torch.optim.SGD(model.parameters(), lr=1e-2).step()
    want = flat0 - torch.tensor(1e-2, dtype=torch.float32, device=DEV) * model.store.grad
    # (torch's own kernel fuses the multiply-add: up to an ulp of the product apart, not bit-equal)
    torch.testing.assert_close(model.store.flat, want, rtol=0, atol=2.0 ** -22 * float(flat0.abs().max()))


# ------------------------------------------------------------------ 5. / 6. the driver
def _editor(compute="f32", vocoder=None):
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    from a3t_amd.sedit import SpeechEditor
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden import fake_phone_duration
    fx, z = _fixture()
    oc = O.tiny_config()
    model, _ = _model(oc, fx["model_seed"], compute)
    fe = LogMelFbank(fs=oc.fs, n_fft=oc.n_fft, win_length=oc.win_length, hop_length=oc.hop_length, n_mels=oc.n_mels,
                     fmin=oc.fmin, fmax=oc.fmax, device=DEV)
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob, mean_phn_span=oc.mean_phn_span,
                        sega_emb=True)
    ids = lambda phns: np.array([fx["token_ids"][ph] for ph in phns], dtype=np.int64)
    phonemise = lambda line: (list(fx["phonemise"][line][0]), dict(fx["phonemise"][line][1]))
    ed = SpeechEditor(model, coll, vocoder, ids, fake_phone_duration)
    new_phns, new_w2p = phonemise(fx["new_str"])
    args = (z["wav"], fx["times2"], fx["word2phns"], new_phns, new_w2p, fx["old_str"], fx["new_str"])
    return ed, args, phonemise, fx, z


def _sample(t, i):
    from make_golden_dyneval import sample_index
    flat = t.reshape(-1)
    return flat[torch.from_numpy(sample_index(i, flat.numel())).to(flat.device)].cpu().numpy()


def test_trajectory_against_the_reference_golden():
    """fp32 compute against the reference's own dynamic_evaluation + prompt_decoding_fn on the fixture (lr 1e-2, 3 steps):
    per-step losses (1e-4 relative) and the step-1 gradient samples (atol 5e-4 * max(1, max|ref|), rtol 5e-3) under the
    bounds of the eval-mode gradient test.

    Total parameter change and adapted mel: the larger of the fixture's own floor and the step-1 gradient bound, times 3 for
    the three steps' compounding.  The floor is measured with the reference alone (its dynamic_evaluation in fp32 against
    fp64, dyneval.json): total change 8.6e-5 relative L2 at worst over the tensors with a non-zero gradient (median 1.7e-6),
    adapted mel 2.4e-6 of its scale -- both below the gradient bound, which therefore sets the tolerance:
      change:  |got - ref| <= 3 * (lr * 5e-4 * max(1, max|grad_ref|)  +  5e-3 * |ref|)   per sampled element
               (one step's change is lr * g, so the gradient's atol scales by lr; `floor * max|ref|` replaces the first term
               where it is larger)
      mel:     max |got - ref| <= 3 * max(floor_mel, 5e-3) * max|mel_ref| = 1.5e-2 of scale, over the generated span; the
               frames outside it are the input log-mel, compared like the SpeechEditor test does (1e-3).
    Measured on MI355X (the test prints the figures): losses 0 / 9.6e-8 / 3.3e-7 relative; step-1 gradient samples at 0.1 %
    of their bound; total change at 0.8 % of its bound at worst, 2.7e-5 relative L2 for the worst tensor's sample; adapted mel
    5.9e-6 of scale (the adaptation itself moves it by 0.65 of scale)."""
    ed, args, phonemise, fx, z = _editor()
    store = ed.model.store
    names = fx["param_names"]
    lr, steps = fx["lr"], fx["steps"]
    loaded = store.flat.clone()
    sd0 = {k: v.clone() for k, v in store.state_dict().items()}
    bufs = _buffers(store)

    # step-1 gradients: what one step leaves in the flat gradient buffer
    l1 = ed.dynamic_evaluation(*args[:3], fx["old_str"], phonemise, lr=lr, steps=1)
    grads = store.state_dict(grads=True)
    ed.restore()
    assert torch.equal(store.flat, loaded)
    worst_g = (0.0, "")
    for i, k in enumerate(names):
        ref = z["grad." + k]
        got = _sample(grads[k], i)
        atol = GRAD_ATOL * max(1.0, float(z["gradmax." + k]))
        worst_g = max(worst_g, (float((np.abs(got - ref) / (atol + GRAD_RTOL * np.abs(ref))).max()), k))
    print(f"step-1 gradient samples: worst error {worst_g[0]:.3f} of the bound ({worst_g[1]})")

    # the whole trajectory, then the decode with the adapted model
    losses = ed.dynamic_evaluation(*args[:3], fx["old_str"], phonemise, lr=lr, steps=steps)
    assert losses.shape == (steps,) and losses.is_cuda
    got_l = losses.cpu().numpy().astype(np.float64)
    rel = np.abs(got_l - np.asarray(fx["losses"])) / np.abs(fx["losses"])
    print(f"losses {got_l.tolist()} reference {fx['losses']} relative error {rel.tolist()}")
    assert float(l1[0]) == got_l[0]
    ed.restore()
    assert torch.equal(store.flat, loaded)
    wav, mel, old_b, new_b = ed.decode(*args, duration_adjust=True, start_end_sp=False, dynamic_eval=(lr, steps),
                                       phonemise_fn=phonemise)
    sd = store.state_dict()                # decode(dynamic_eval=...) leaves the model adapted until restore()
    ed.restore()
    assert torch.equal(store.flat, loaded)
    for k, v in _buffers(store).items():
        assert torch.equal(v, bufs[k]), k
    worst_d, rel_l2 = (0.0, ""), (0.0, "")
    for i, k in enumerate(names):
        ref = z["delta." + k]
        got = _sample(sd[k] - sd0[k], i)
        atol = 3 * max(lr * GRAD_ATOL * max(1.0, float(z["gradmax." + k])), fx["floor_delta"][k] * float(np.abs(ref).max()))
        worst_d = max(worst_d, (float((np.abs(got - ref) / (atol + 3 * GRAD_RTOL * np.abs(ref))).max()), k))
        if float(np.linalg.norm(ref)) > 1e-6:
            rel_l2 = max(rel_l2, (float(np.linalg.norm(got - ref) / np.linalg.norm(ref)), k))
    print(f"total change: worst error {worst_d[0]:.3f} of the bound ({worst_d[1]}); worst relative L2 of a sample "
          f"{rel_l2[0]:.2e} ({rel_l2[1]}); the reference's own fp32-vs-fp64 floor {fx['floor_delta_max']:.2e}")
    got_mel, ref_mel = mel.cpu().numpy(), z["mel"]
    assert [int(x) for x in old_b] == fx["old_span_boundary"] and [int(x) for x in new_b] == fx["new_span_boundary"]
    assert got_mel.shape == ref_mel.shape == (fx["mel_frames"], 80)
    s, e = fx["new_span_boundary"]
    scale = float(np.abs(ref_mel).max())
    mel_err = float(np.abs(got_mel[s:e] - ref_mel[s:e]).max()) / scale
    print(f"adapted mel: max error {mel_err:.2e} of scale (floor {fx['floor_mel']:.2e}; the adaptation moved it by "
          f"{fx['mel_moved']:.2e} of scale)")

    assert (rel < LOSS_RTOL).all(), rel
    assert worst_g[0] <= 1.0, worst_g
    assert worst_d[0] <= 1.0, worst_d
    assert mel_err <= 3 * max(fx["floor_mel"], GRAD_RTOL), mel_err
    np.testing.assert_allclose(got_mel[:s], ref_mel[:s], atol=1e-3, rtol=1e-3)
    np.testing.assert_allclose(got_mel[e:], ref_mel[e:], atol=1e-3, rtol=1e-3)


def test_prompt_tts_driver():
    """SpeechEditor.prompt_tts: the crop of prompt_decoding_fn, dynamic_eval=(0, 0) = decode bit for bit, the parameters back
    at the loaded checkpoint after every call, and adaptation at a well-resolved lr (the fixture's, at which the reference's
    own losses fall) lowers the masked-reconstruction loss of the prompt batch from step to step."""
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    cfg = O.PWGConfig()
    vstate = O.procedural_state(O.pwg_param_shapes(cfg), seed=4)
    for k in vstate:
        if "up_layers" in k:
            vstate[k] = np.abs(vstate[k]) / np.abs(vstate[k]).sum()
    voc = ParallelWaveGANGeneratorHIP(vstate, device=DEV)
    hop = O.tiny_config().hop_length

    def vocoder(feat):
        noise = torch.from_numpy(np.random.RandomState(9).standard_normal((feat.shape[0] * hop, 1)).astype(np.float32))
        return voc.inference(feat, noise)

    ed, args, phonemise, fx, z = _editor(vocoder=vocoder)
    store = ed.model.store
    loaded = store.flat.clone()
    bufs = _buffers(store)
    _, mel_plain, old_b, new_b = ed.decode(*args, duration_adjust=True, start_end_sp=False)
    res = ed.prompt_tts(*args)
    assert set(res) == {"prompt", "new_wav", "feat", "old_span_boundary", "new_span_boundary"}
    assert torch.equal(res["feat"], mel_plain) and res["new_span_boundary"] == new_b == fx["new_span_boundary"]
    assert res["prompt"] is not None and np.array_equal(res["prompt"], z["wav"])
    full = vocoder(res["feat"]).detach().float().reshape(-1).cpu().numpy()
    T_new = res["feat"].shape[0]
    assert res["new_wav"].shape == (hop * (T_new - new_b[0]),) == (fx["new_wav_len"],)
    assert np.array_equal(res["new_wav"], full[hop * new_b[0]:])
    np.testing.assert_allclose(mel_plain.cpu().numpy(), z["mel_unadapted"], atol=1e-3, rtol=1e-3)
    assert torch.equal(store.flat, loaded)

    # with dynamic evaluation: another mel, the same parameters afterwards
    res2 = ed.prompt_tts(*args, dynamic_eval=(fx["lr"], fx["steps"]), phonemise_fn=phonemise)
    assert torch.equal(store.flat, loaded) and ed._loaded is None
    s, e = new_b
    assert res2["feat"].shape == mel_plain.shape and not torch.equal(res2["feat"][s:e], mel_plain[s:e])
    assert torch.equal(res2["feat"][:s], mel_plain[:s])
    assert res2["new_wav"].shape == res["new_wav"].shape
    with pytest.raises(ValueError, match="phonemise_fn"):
        ed.prompt_tts(*args, dynamic_eval=(fx["lr"], 1))
    # edit() offers the same argument and restores too
    res3 = ed.edit(*args, dynamic_eval=(fx["lr"], fx["steps"]), phonemise_fn=phonemise)
    # (two adaptations are not bit-identical: the backward accumulates some gradients with atomics)
    torch.testing.assert_close(res3["feat"], res2["feat"], atol=1e-3, rtol=1e-3)
    assert torch.equal(store.flat, loaded)

    # the adaptation itself, and the context manager
    with ed:
        losses = ed.dynamic_evaluation(*args[:3], fx["old_str"], phonemise, lr=fx["lr"], steps=fx["steps"]).cpu().numpy()
        assert not torch.equal(store.flat, loaded)
    assert torch.equal(store.flat, loaded)
    print("losses", losses.tolist())
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    for k, v in _buffers(store).items():
        assert torch.equal(v, bufs[k]), k
    ed.model.train()
    with pytest.raises(TypeError):
        ed.dynamic_evaluation(*args[:3], fx["old_str"], phonemise)
