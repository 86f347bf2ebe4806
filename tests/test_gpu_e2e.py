"""End-to-end GPU parity: the HIP training step (forward, loss, full backward, optimiser) against
the golden vectors produced by the reference and against the CPU oracle."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"


def _engine(oc, seed, compute="f32", training=True):
    from a3t_amd.config import A3TConfig
    from a3t_amd.engine import MLMEngine
    from a3t_amd.params import ParamStore
    c = A3TConfig(**{k: getattr(oc, k) for k in ("idim", "odim", "vocab", "adim", "heads", "ff", "ff_kernel",
                                                  "enc_blocks", "dec_blocks", "enc_kernel", "dec_kernel",
                                                  "postnet_layers", "postnet_chans", "postnet_filts", "max_len",
                                                  "seg_table", "lsm_weight")})
    store = ParamStore(c, DEV)
    state = O.procedural_state(O.param_shapes(oc), seed)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    return MLMEngine(c, store, compute=compute, training=training), store


def _to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def test_state_dict_roundtrip():
    oc = O.tiny_config()
    eng, store = _engine(oc, 1)
    sd = store.state_dict()
    ref = O.procedural_state(O.param_shapes(oc), 1)
    assert set(sd.keys()) == set(ref.keys())
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(np.shape(v)), k
        np.testing.assert_array_equal(sd[k].cpu().numpy(), v, err_msg=k)


def test_e2e_tiny_against_reference_golden():
    g = np.load(os.path.join(G, "e2e_tiny.npz"))
    oc = O.tiny_config()
    batch = O.synthetic_batch(oc, B=2, T_mel=48, T_phn=8, seed=11, lengths=[48, 37], text_lengths=[8, 6])
    eng, store = _engine(oc, 1)
    out = eng.forward(_to_dev(batch))
    loss = float(out["loss"])
    assert abs(loss - float(np.asarray(g["loss"]).reshape(-1)[0])) < 1e-4 * abs(float(np.asarray(g["loss"]).reshape(-1)[0]))   # 1e-4 relative on the summed loss
    np.testing.assert_allclose(out["before"].cpu().numpy(), g["before"], atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out["after"].cpu().numpy(), g["after"], atol=2e-4, rtol=1e-4)
    store.zero_grad()
    eng.backward()
    grads = store.state_dict(grads=True)
    for k in g.files:
        if not k.startswith("grad."):
            continue
        n = k[5:]
        ref = g[k]
        got = grads[n].cpu().numpy()
        np.testing.assert_allclose(got, ref, atol=5e-4 * max(1.0, float(np.abs(ref).max())), rtol=5e-3, err_msg=n)
    sd = store.state_dict()
    for k in g.files:
        if k.startswith("buf.") and "running" in k:
            np.testing.assert_allclose(sd[k[4:]].cpu().numpy(), g[k], atol=1e-5, rtol=1e-4, err_msg=k)
    # eval-mode BN (running statistics) forward
    eng_e, _ = _engine(oc, 1, training=False)
    le = float(eng_e.forward(_to_dev(batch), need_grad=False)["loss"])
    assert abs(le - float(g["loss_eval"])) < 1e-4 * abs(float(g["loss_eval"]))


def test_e2e_reference_yaml_config():
    g = np.load(os.path.join(G, "e2e_refyaml.npz"))
    oc = O.A3TConfig()
    batch = O.synthetic_batch(oc, B=2, T_mel=200, T_phn=30, seed=12, lengths=[200, 163], text_lengths=[30, 24])
    eng, store = _engine(oc, 3)
    assert store.n_params == int(g["n_params"])
    out = eng.forward(_to_dev(batch))
    assert abs(float(out["loss"]) - float(np.asarray(g["loss"]).reshape(-1)[0])) < 1e-4 * abs(float(np.asarray(g["loss"]).reshape(-1)[0]))
    np.testing.assert_allclose(out["before"].cpu().numpy(), g["before"], atol=5e-4, rtol=1e-3)
    np.testing.assert_allclose(out["after"].cpu().numpy(), g["after"], atol=5e-4, rtol=1e-3)
    store.zero_grad()
    eng.backward()
    grads = store.state_dict(grads=True)
    for n, gn in zip(g["grad_names"], g["grad_norm"]):
        got = float(grads[str(n)].double().norm())
        assert abs(got - gn) <= 5e-3 * max(gn, 1e-2), (n, got, gn)


def test_e2e_bf16_compute_within_1e2():
    """bf16 MFMA compute path: loss within 1e-2 relative of the fp32 oracle (north_star tolerance)."""
    oc = O.A3TConfig(enc_blocks=2, dec_blocks=2)
    batch = O.synthetic_batch(oc, B=2, T_mel=200, T_phn=24, seed=5)
    p = O.to_torch_state(O.procedural_state(O.param_shapes(oc), 7))
    with torch.no_grad():
        ref, _, _ = O.forward_loss(p, batch, oc, True)
    eng, store = _engine(oc, 7, compute="bf16")
    out = eng.forward(_to_dev(batch))
    assert abs(float(out["loss"]) - float(ref)) < 1e-2 * abs(float(ref))
    store.zero_grad()
    eng.backward()
    assert torch.isfinite(store.grad).all()
    # every parameter gradient of the bf16 path (fused bias sums, bf16 operands) against the fp32 path
    eng32, store32 = _engine(oc, 7, compute="f32")
    eng32.forward(_to_dev(batch))
    store32.zero_grad()
    eng32.backward()
    g16, g32 = store.state_dict(grads=True), store32.state_dict(grads=True)
    bad = []
    for k in g32:
        a, b = g16[k].double().flatten(), g32[k].double().flatten()
        nb = float(b.norm())
        if nb < 1e-6 or k.endswith("depthwise_conv.bias"):   # a bias in front of BatchNorm: gradient is analytically 0
            continue
        cos = float((a * b).sum() / (a.norm() * b.norm() + 1e-30))
        ratio = float(a.norm()) / nb
        if cos < 0.97 or not (0.9 < ratio < 1.1):
            bad.append((k, round(cos, 4), round(ratio, 4)))
    assert not bad, bad[:10]


def _task_args(oc):
    import argparse
    enc = dict(input_layer="sega_mlm", cnn_module_kernel=oc.enc_kernel, attention_dim=oc.adim, attention_heads=oc.heads,
               linear_units=oc.ff, num_blocks=oc.enc_blocks, macaron_style=True, use_cnn_module=True,
               selfattention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos", positionwise_layer_type="conv1d",
               positionwise_conv_kernel_size=3)
    dec = dict(cnn_module_kernel=oc.dec_kernel, attention_dim=oc.adim, attention_heads=oc.heads, linear_units=oc.ff,
               num_blocks=oc.dec_blocks, selfattention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos")
    mc = dict(lsm_weight=0.1, mean_phn_span=8, mlm_prob=0.8, postnet_layers=oc.postnet_layers, postnet_filts=5,
              postnet_chans=oc.postnet_chans, dropout=False)   # parity tests: deterministic train-mode engine
    return argparse.Namespace(token_list=[f"t{i}" for i in range(oc.vocab)], odim=80, input_size=80,
                              feats_extract="fbank", feats_extract_conf=dict(n_fft=2048, hop_length=300,
                                                                             win_length=1200, fs=24000, fmin=80,
                                                                             fmax=7600, n_mels=80),
                              normalize=None, normalize_conf={}, encoder="conformer", encoder_conf=enc,
                              decoder="conformer", decoder_conf=dec, model_conf=mc, init=None)


def test_plugin_model_loss_backward_and_inference():
    """The ESPnet2 model surface: forward(**batch) -> (loss, stats, weight); loss.backward() fills p.grad."""
    from a3t_amd.task import MLMTask
    g = np.load(os.path.join(G, "e2e_tiny.npz"))
    oc = O.tiny_config()
    model = MLMTask.build_model(_task_args(oc), device=DEV)
    state = O.procedural_state(O.param_shapes(oc), 1)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    batch = O.synthetic_batch(oc, B=2, T_mel=48, T_phn=8, seed=11, lengths=[48, 37], text_lengths=[8, 6])
    model.train()
    loss, stats, weight = model(**batch)
    assert loss.shape == (1,) and weight.tolist() == [2] and set(stats) == {"loss", "loss_mlm", "loss_copy"}
    assert abs(float(loss) - float(np.asarray(g["loss"]).reshape(-1)[0])) < 1e-4 * abs(float(np.asarray(g["loss"]).reshape(-1)[0]))
    (loss * 2.0).backward()                       # the trainer rescales the loss (world_size / accum_grad)
    grads = model.store.state_dict(grads=True)    # flat buffer == what autograd accumulated into p.grad
    name = "encoder.encoders.0.feed_forward.w_1.weight"
    np.testing.assert_allclose(grads[name].cpu().numpy(), 2.0 * g["grad." + name], atol=2e-3, rtol=1e-2)
    pgrad = dict(model.named_parameters())["enc__0__ff__w1"].grad        # kernel layout [ff][tap][d]
    np.testing.assert_allclose(pgrad.permute(0, 2, 1).cpu().numpy(), 2.0 * g["grad." + name], atol=2e-3, rtol=1e-2)
    # teacher-forced infill (sedit_model.py:274-284), eval-mode BN
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    b1 = {k: v[:1] for k, v in batch.items()}
    with torch.no_grad():
        out = model.inference(**b1, span_boundary=[10, 30], use_teacher_forcing=True)
    sp = torch.cat([out["feat_gen"][0][0], out["feat_gen"][1], out["feat_gen"][2][0]], dim=0)
    np.testing.assert_allclose(sp.cpu().numpy(), g["infer_splice"], atol=2e-4, rtol=1e-3)


def test_logmel_and_collate_on_device():
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    g = np.load(os.path.join(G, "logmel.npz"))
    fe = LogMelFbank(fs=24000, n_fft=2048, win_length=1200, hop_length=300, n_mels=80, fmin=80, fmax=7600, device=DEV)
    feats, flen = fe(torch.from_numpy(g["wav"]), torch.from_numpy(g["lens"]))
    assert np.array_equal(flen.cpu().numpy(), g["feats_lengths"])
    np.testing.assert_allclose(feats.cpu().numpy(), g["feats"], atol=2e-4, rtol=0)
    c = np.load(os.path.join(G, "collate.npz"))
    data = [(f"utt{i}", {k: c[f"in{i}.{k}"] for k in ("speech", "text", "align_start", "align_end")}) for i in range(2)]
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=0.8, mean_phn_span=8, sega_emb=True)
    np.random.seed(77)
    uids, b = coll(data)
    assert uids == ["utt0", "utt1"]
    for k in ("text", "masked_position", "speech_mask", "text_mask", "speech_segment_pos", "text_segment_pos",
              "speech_lengths", "text_lengths"):
        assert np.array_equal(b[k].numpy(), c["out." + k]), k
    np.testing.assert_allclose(b["speech"].numpy(), c["out.speech"], atol=2e-4)


def test_collate_on_device_matches_host_collate_bit_for_bit():
    """device_out=True (round 4): features stay on the device, masks / segment ids / padding masks are painted
    by a3t_collate_paint from the integer span lists; only the numpy-RNG draws run on the host.  Against the reference's own
    MLMCollateFn output (collate.npz) and against the host path on ragged random batches, all four masking branches."""
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    fe = LogMelFbank(fs=24000, n_fft=2048, win_length=1200, hop_length=300, n_mels=80, fmin=80, fmax=7600, device=DEV)
    c = np.load(os.path.join(G, "collate.npz"))
    data = [(f"utt{i}", {k: c[f"in{i}.{k}"] for k in ("speech", "text", "align_start", "align_end")}) for i in range(2)]
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=0.8, mean_phn_span=8, sega_emb=True, device_out=True)
    np.random.seed(77)
    uids, b = coll(data)
    assert uids == ["utt0", "utt1"] and all(v.is_cuda for v in b.values())
    for k in ("text", "masked_position", "speech_mask", "text_mask", "speech_segment_pos", "text_segment_pos",
              "speech_lengths", "text_lengths"):
        assert b[k].dtype == torch.from_numpy(c["out." + k]).dtype, k
        assert np.array_equal(b[k].cpu().numpy(), c["out." + k]), k
    np.testing.assert_allclose(b["speech"].cpu().numpy(), c["out.speech"], atol=2e-4)
    rs = np.random.RandomState(8)
    hop, fs = 300, 24000
    for case in range(8):
        B = int(rs.randint(1, 6))
        data = []
        for i in range(B):
            F_ = int(rs.randint(30, 120))
            n = hop * (F_ - 1) + int(rs.randint(0, hop))
            P = int(rs.randint(1, 14))
            cuts = np.sort(rs.choice(np.arange(1, F_ - 1), P - 1, replace=False)) if P > 1 else np.zeros(0, np.int64)
            st = np.concatenate([[0], cuts]).astype(np.float64) * hop / fs + 1e-4
            en = np.concatenate([cuts, [F_ - 1]]).astype(np.float64) * hop / fs + 1e-4
            d = dict(speech=(0.1 * rs.standard_normal(n)).astype(np.float32), text=rs.randint(2, 70, size=P).astype(np.int64),
                     align_start=st.astype(np.float32), align_end=en.astype(np.float32))
            if case % 4 == 1:
                d["span_boundary"] = np.sort(rs.randint(0, F_, size=2)).astype(np.int64)
            data.append((f"u{i}", d))
        if case % 4 == 1 and len({len(d) for _, d in data}) != 1:
            continue
        kw = dict(mlm_prob=1.0) if case % 4 == 3 else dict(mlm_prob=0.3, mean_phn_span=0) if case % 4 == 2 else dict(mlm_prob=0.8, mean_phn_span=8)
        host = MLMCollateFn(fe, sega_emb=(case % 2 == 0), **kw)
        devc = MLMCollateFn(fe, sega_emb=(case % 2 == 0), device_out=True, **kw)
        np.random.seed(100 + case)
        _, bh = host(data)
        st_h = np.random.get_state()[1].copy()
        np.random.seed(100 + case)
        _, bd = devc(data)
        assert np.array_equal(np.random.get_state()[1], st_h)
        for k in bh:
            assert bd[k].dtype == bh[k].dtype and tuple(bd[k].shape) == tuple(bh[k].shape), (case, k)
            if k == "speech":
                np.testing.assert_allclose(bd[k].cpu().numpy(), bh[k].numpy(), atol=1e-6)
            else:
                assert np.array_equal(bd[k].cpu().numpy(), bh[k].numpy()), (case, k)


def test_dropout_backward_matches_finite_differences():
    """With dropout on (counter RNG, fixed step seed) the loss is a deterministic function of the
    parameters: the hand-written backward must agree with a central finite difference along the
    gradient direction.  fp32 engine, reference-architecture tiny config."""
    from a3t_amd.config import A3TConfig
    from a3t_amd.engine import MLMEngine
    from a3t_amd.params import ParamStore
    oc = O.tiny_config()
    c = A3TConfig(adim=oc.adim, heads=oc.heads, ff=oc.ff, enc_blocks=1, dec_blocks=1, postnet_layers=2,
                  postnet_chans=16, vocab=oc.vocab, dropout_rate=0.2, positional_dropout_rate=0.2,
                  attention_dropout_rate=0.2, postnet_dropout_rate=0.5)
    store = ParamStore(c, DEV)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in O.procedural_state(O.param_shapes(oc), 1).items()})
    eng = MLMEngine(c, store, compute="f32", training=True, dropout=True)
    batch = _to_dev(O.synthetic_batch(oc, B=2, T_mel=48, T_phn=8, seed=11))

    def loss_at(theta):
        store.flat.copy_(theta)
        eng.step_seed = 41                      # same masks every evaluation
        return float(eng.forward(batch, need_grad=False)["loss"])

    theta0 = store.flat.clone()
    eng.step_seed = 41
    l0 = float(eng.forward(batch)["loss"])
    store.zero_grad()
    eng.backward()
    g = store.grad.clone()
    # dropout really is on: a different seed gives a different loss
    eng.step_seed = 5
    assert abs(float(eng.forward(batch, need_grad=False)["loss"]) - l0) > 1e-3
    v = g / g.norm()
    eps = 2e-3
    fd = (loss_at(theta0 + eps * v) - loss_at(theta0 - eps * v)) / (2 * eps)
    an = float((g * v).sum())
    assert abs(fd - an) < 3e-2 * abs(an), (fd, an)
    # BatchNorm running stats must not matter for the train-mode loss; restore parameters
    store.flat.copy_(theta0)


@pytest.mark.parametrize("fused", [True, False])
def test_parallel_wavegan_generator_matches_vendored_reference(fused):
    """fused=True: two fp32-MFMA kernels per residual block (pwg_fused.hip); False: layer-by-layer GEMM path."""
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    g = np.load(os.path.join(G, "pwg.npz"))
    cfg = O.PWGConfig()
    state = O.procedural_state(O.pwg_param_shapes(cfg), seed=4)
    for k in state:
        if "up_layers" in k:
            state[k] = np.abs(state[k]) / np.abs(state[k]).sum()
    voc = ParallelWaveGANGeneratorHIP(state, device=DEV, fused=fused)
    assert voc.fused == fused
    wav = voc.inference(torch.from_numpy(g["c"]), torch.from_numpy(g["z"]))
    assert wav.shape == (6000, 1)
    np.testing.assert_allclose(wav.cpu().numpy(), g["wav"], atol=2e-5, rtol=1e-4)
    # batched call = independent utterances
    wb = voc.inference(torch.from_numpy(g["c"])[None].repeat(2, 1, 1), torch.from_numpy(g["z"])[None].repeat(2, 1, 1))
    np.testing.assert_allclose(wb[1].cpu().numpy(), g["wav"], atol=2e-5, rtol=1e-4)


def test_bf16_schedule_side_stream_and_fused_dropout_match_serial_schedule():
    """The production bf16 backward (weight-gradient GEMMs on the side stream, scratch double-buffered by sub-layer
    parity, LayerNorm backward emitting the next sub-layer's dropout-masked operand) must give the gradients of the
    plain one-stream schedule with the separate dropout pass: same seeds, d = 128 so every fast path is taken."""
    from a3t_amd.config import A3TConfig
    from a3t_amd.engine import MLMEngine
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    c = A3TConfig(adim=128, heads=2, ff=256, enc_blocks=2, dec_blocks=2, postnet_layers=3, postnet_chans=64, vocab=40,
                  dropout_rate=0.2, positional_dropout_rate=0.2, attention_dropout_rate=0.2, postnet_dropout_rate=0.5)
    store = ParamStore(c, DEV)
    xavier_init_(store, seed=3, bn_gamma=1.0)
    from a3t_amd.collate import synthetic_batch
    batch = synthetic_batch(c, 4, 192, 32, seed=7, device=DEV)
    grads = []
    for fast in (True, False, True):
        eng = MLMEngine(c, store, compute="bf16", training=True, dropout=True)
        if not fast:
            eng.side = None
            eng.opt.fuse_ln_dropout = False
        eng.step_seed = 9
        eng.refresh_weights()
        store.zero_grad()
        loss = float(eng.forward(batch)["loss"])
        eng.backward()
        torch.cuda.synchronize()
        grads.append((loss, store.grad.clone()))
    assert grads[0][0] == grads[1][0]
    ref = grads[1][1]
    for loss, g in (grads[0], grads[2]):
        err = float((g - ref).abs().max() / ref.abs().max())
        assert err < 2e-4, err          # only the order of fp32 atomics differs
        assert float(torch.nn.functional.cosine_similarity(g, ref, dim=0)) > 0.999999


def test_grouped_weight_gradients_on_a_shallow_scratch_ring_match_single_launches(monkeypatch):
    """ADVICE r5 (ConformerStack._wg_flush): collected Linear weight gradients are handed over after their sub-layer ended; with the
    shallowest ring that still groups (A3T_SIDE_DEPTH=8) the main stream reuses a scratch set 8 sub-layers later and must
    wait for the GROUP launch that reads it, not only for the work issued inside the sub-layer.  16 blocks = 80 sub-layers:
    ten laps of the ring; dropout on so that the operands live in tmp.gm / tmp.dg.  Equal to one launch per gradient."""
    from a3t_amd.config import A3TConfig
    from a3t_amd.engine import MLMEngine
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    from a3t_amd.collate import synthetic_batch
    if os.environ.get("A3T_SIDE_STREAM") == "0":
        pytest.skip("one-stream schedule (A3T_SIDE_STREAM=0): nothing is grouped or handed over")
    c = A3TConfig(adim=384, heads=2, ff=768, enc_blocks=8, dec_blocks=8, postnet_layers=3, postnet_chans=64, vocab=40,
                  dropout_rate=0.2, positional_dropout_rate=0.2, attention_dropout_rate=0.2, postnet_dropout_rate=0.5)
    store = ParamStore(c, DEV)
    xavier_init_(store, seed=3, bn_gamma=1.0)
    batch = synthetic_batch(c, 8, 512, 64, seed=7, device=DEV)
    grads = []
    for depth, group in (("8", "1"), ("48", "0"), ("8", "1")):
        monkeypatch.setenv("A3T_SIDE_DEPTH", depth)
        monkeypatch.setenv("A3T_WGRAD_GROUP", group)
        eng = MLMEngine(c, store, compute="bf16", training=True, dropout=True)
        assert eng._wg_group == (4 if group == "1" else 1) and eng._depth == int(depth)
        eng.step_seed = 9
        store.zero_grad()
        loss = float(eng.forward(batch)["loss"])
        eng.backward()
        torch.cuda.synchronize()
        grads.append((loss, store.grad.clone()))
        del eng
    assert grads[0][0] == grads[1][0]
    ref = grads[1][1]
    for loss, g in (grads[0], grads[2]):
        err = float((g - ref).abs().max() / ref.abs().max())
        assert err < 2e-4, err
        assert float(torch.nn.functional.cosine_similarity(g, ref, dim=0)) > 0.999999


def test_bare_conformer_stack_gives_the_engines_block_bit_for_bit():
    """A ConformerStack with no model around it (what the FastSpeech2 models build) and an MLMEngine run the same block on the
    same store and input: the same launches, so the same bits -- for a plain batch and for one whose second row is shorter."""
    from a3t_amd.config import A3TConfig
    from a3t_amd.conformer import ConformerStack
    from a3t_amd.engine import MLMEngine
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    c = A3TConfig(adim=128, heads=2, ff=256, enc_blocks=1, dec_blocks=1, postnet_layers=2, postnet_chans=32, vocab=40)
    store = ParamStore(c, DEV)
    xavier_init_(store, seed=3, bn_gamma=1.0)
    B, T = 2, 16
    x = torch.randn(B * T, c.adim, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    keymask = torch.ones(B, T, dtype=torch.uint8, device=DEV)
    stack = ConformerStack(c, store, compute="f32", training=False)
    eng = MLMEngine(c, store, compute="f32", training=False)
    assert not isinstance(stack, MLMEngine) and stack.ws is not eng.ws
    for lens in (None, torch.tensor([T, T - 5], dtype=torch.int32, device=DEV)):
        outs = []
        for e in (stack, eng):
            y = e.block_fwd("enc.0", x, e.pe[:T], keymask, B, T, lens=lens)
            outs.append(e._ln_fwd("enc.after", y, "enc.after", out_dtype=torch.float32).clone())
        torch.cuda.synchronize()
        n = B * T if lens is None else B * T - 5       # (rows behind a length hold values nobody reads: the tail of row 1)
        assert bool(torch.isfinite(outs[0][:n]).all()) and float(outs[0][:n].abs().max()) > 0
        assert torch.equal(outs[0][:n], outs[1][:n])


def test_trainer_overlapped_allreduce_plumbing_single_rank_rccl():
    """The data-parallel step on real RCCL with a 1-rank group: bucketed all-reduce on its own stream, fired from
    the backward hooks after the engine's side stream has drained.  A 1-rank SUM is the identity, so the reduced
    gradient of step 1 and the loss of step 2 must equal those of the plain (no process group) trainer (parameters
    themselves are not compared: Adam's first steps are +-lr*sign(g), so fp32-atomic-order noise on near-zero
    gradients flips individual updates)."""
    import torch.distributed as dist
    from a3t_amd.config import A3TConfig
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    from a3t_amd.trainer import A3TTrainer
    from a3t_amd.collate import synthetic_batch
    c = A3TConfig(adim=128, heads=2, ff=256, enc_blocks=2, dec_blocks=2, postnet_layers=3, postnet_chans=64, vocab=40)
    batch = synthetic_batch(c, 4, 192, 32, seed=7, device=DEV)

    def run(with_group):
        store = ParamStore(c, DEV)
        xavier_init_(store, seed=3, bn_gamma=1.0)
        tr = A3TTrainer(c, store, compute="bf16", lr=1.0, warmup_steps=10, dropout=True, force_reducer=with_group,
                        bucket_min_elems=200_000)
        if with_group:
            assert tr.reducer is not None and len(tr.reducer.ranges) >= 3      # several buckets, fired from the hooks
        l1 = float(tr.step(batch))
        torch.cuda.synchronize()
        g1 = store.grad.clone()
        l2 = float(tr.step(batch))
        torch.cuda.synchronize()
        return (l1, l2), g1

    ref_l, ref_p = run(False)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV, 0))
    try:
        got_l, got_p = run(True)
    finally:
        dist.destroy_process_group()
    assert abs(got_l[0] - ref_l[0]) < 1e-5 * abs(ref_l[0])
    assert abs(got_l[1] - ref_l[1]) < 2e-3 * abs(ref_l[1])
    err = float((got_p - ref_p).abs().max() / ref_p.abs().max())
    assert err < 2e-4, err
    assert float(torch.nn.functional.cosine_similarity(got_p, ref_p, dim=0)) > 0.999999


def _engine_for(c, compute, seed=3, dropout=False):
    from a3t_amd.engine import MLMEngine
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    store = ParamStore(c, DEV)
    xavier_init_(store, seed=seed, bn_gamma=1.0)
    return store, MLMEngine(c, store, compute=compute, training=True, dropout=dropout)


def test_size_independent_properties_bf16():
    """Properties the path must have at any size (checked at d=384, B=6, T=488 on the bf16 production schedule):
    (1) permuting the utterances of the batch permutes the outputs and leaves the loss unchanged (train-mode BatchNorm
    and the masked mean are symmetric in the batch); (2) the backward is linear in the loss scale; (3) an utterance
    with no masked frame contributes no loss and a fully masked one is handled (denominator = masked frames)."""
    from a3t_amd.config import A3TConfig
    from a3t_amd.collate import synthetic_batch
    c = A3TConfig(enc_blocks=1, dec_blocks=1)
    store, eng = _engine_for(c, "bf16")
    batch = synthetic_batch(c, 6, 440, 48, seed=5, device=DEV)
    batch["masked_position"][0] = False
    batch["masked_position"][1] = True
    eng.refresh_weights()
    store.zero_grad()
    out = eng.forward(batch)
    loss, after = float(out["loss"]), out["after"].clone()
    eng.backward()
    g1 = store.grad.clone()
    assert math.isfinite(loss) and bool(torch.isfinite(g1).all())
    perm = torch.tensor([3, 0, 5, 1, 4, 2], device=DEV)
    pb = {k: v[perm].contiguous() for k, v in batch.items()}
    out_p = eng.forward(pb, need_grad=False)
    assert abs(float(out_p["loss"]) - loss) < 2e-3 * abs(loss)
    a, b = out_p["after"].float(), after[perm].float()          # bf16 path: only rounding / atomic-order noise may differ
    assert float((a - b).norm() / b.norm()) < 1e-2           # (one-ulp bf16 flips downstream of the BatchNorm sums)
    assert float((a - b).abs().max()) < 0.25
    # the same property on the exact-fp32 engine is tight
    from a3t_amd.engine import MLMEngine
    e32 = MLMEngine(c, store, compute="f32", training=True, dropout=False)
    o1 = e32.forward(batch, need_grad=False)
    l32, a32 = float(o1["loss"]), o1["after"].clone()
    o2 = e32.forward(pb, need_grad=False)
    assert abs(float(o2["loss"]) - l32) < 1e-5 * abs(l32)
    assert float((o2["after"] - a32[perm]).abs().max()) < 2e-3 * float(a32.abs().max())
    store.zero_grad()
    eng.forward(batch, gscale=2.0)
    eng.backward()
    err = float((store.grad - 2.0 * g1).abs().max() / g1.abs().max())
    assert err < 5e-3, err
    # loss = masked mean: zeroing the inputs of the un-masked utterance's target cannot change the loss
    b2 = {k: v.clone() for k, v in batch.items()}
    b2["masked_position"][1] = False                 # fewer masked frames -> different denominator, still finite
    assert math.isfinite(float(eng.forward(b2, need_grad=False)["loss"]))


def test_full_size_c2_step_is_finite_and_bf16_tracks_fp32():
    """BASELINE configs[1] at full size (6+6 blocks, B=32, T_mel=1000, T_phn=120): one bf16 training step gives a
    finite loss and a finite, everywhere-populated gradient; the loss agrees with the fp32 engine to 1e-2."""
    from a3t_amd.config import config_c2
    from a3t_amd.collate import synthetic_batch
    c = config_c2()
    store, eng = _engine_for(c, "bf16")
    batch = synthetic_batch(c, 32, 1000, 120, seed=1234, device=DEV)
    eng.refresh_weights()
    store.zero_grad()
    loss16 = float(eng.forward(batch)["loss"])
    eng.backward()
    torch.cuda.synchronize()
    assert math.isfinite(loss16) and bool(torch.isfinite(store.grad).all())
    dead = [n for n, g in store.g.items() if float(g.abs().max()) == 0.0 and not n.endswith(".db")]
    assert not dead, dead
    del eng
    torch.cuda.empty_cache()
    from a3t_amd.engine import MLMEngine
    e32 = MLMEngine(c, store, compute="f32", training=True, dropout=False)
    loss32 = float(e32.forward(batch, need_grad=False)["loss"])
    assert abs(loss16 - loss32) < 1e-2 * abs(loss32), (loss16, loss32)


def test_c4_shape_family_bf16_tracks_fp32():
    """BASELINE configs[3] architecture family (d=512, H=4 -> d_k=128, ff=2048) at a small batch: every kernel sees
    shapes different from the recipe's (LayerNorm D=512, attention N=128 tiles, 4 heads per utterance).  The bf16
    production schedule must track the exact-fp32 engine: loss to 1e-2, flat gradient cosine >= 0.99."""
    from a3t_amd.config import A3TConfig
    from a3t_amd.collate import synthetic_batch
    from a3t_amd.engine import MLMEngine
    c = A3TConfig(adim=512, heads=4, ff=2048, enc_blocks=2, dec_blocks=2)
    store, eng = _engine_for(c, "bf16")
    batch = synthetic_batch(c, 3, 400, 48, seed=21, device=DEV)
    eng.refresh_weights()
    store.zero_grad()
    l16 = float(eng.forward(batch)["loss"])
    eng.backward()
    torch.cuda.synchronize()
    g16 = store.grad.clone()
    e32 = MLMEngine(c, store, compute="f32", training=True, dropout=False)
    store.zero_grad()
    l32 = float(e32.forward(batch)["loss"])
    e32.backward()
    torch.cuda.synchronize()
    g32 = store.grad.clone()
    assert abs(l16 - l32) < 1e-2 * abs(l32), (l16, l32)
    assert bool(torch.isfinite(g16).all())
    assert float(torch.nn.functional.cosine_similarity(g16, g32, dim=0)) > 0.99
    assert abs(float(g16.norm() / g32.norm()) - 1.0) < 0.05


def test_plugin_model_bf16_accepts_arbitrary_lengths():
    """compute='bf16' needs T_mel and T_mel + T_phn to be multiples of 8; the plugin model extends the batch padding
    itself (masked-out frames / pad phones, as the reference's collate does for a longer batch).  The bf16 model on odd
    lengths must agree with the fp32 model fed the explicitly padded batch, train and infer."""
    from a3t_amd.task import MLMTask
    from a3t_amd.espnet_model import ESPnetMLMEncAsDecoderModel
    oc = O.A3TConfig(enc_blocks=1, dec_blocks=1)
    state = O.procedural_state(O.param_shapes(oc), 1)
    sd = {k: torch.from_numpy(np.array(v)) for k, v in state.items()}
    batch = O.synthetic_batch(oc, B=2, T_mel=203, T_phn=31, seed=11, lengths=[203, 150], text_lengths=[31, 20])
    m16 = MLMTask.build_model(_task_args(oc), device=DEV, compute="bf16")
    m16.load_state_dict(sd)
    m32 = MLMTask.build_model(_task_args(oc), device=DEV, compute="f32")
    m32.load_state_dict(sd)
    m16.train(), m32.train()
    l16, _, w = m16(**batch)
    l16.backward()
    padded = ESPnetMLMEncAsDecoderModel._pad_to_dma_granule({k: v.to(DEV) for k, v in batch.items() if k in (
        "speech", "text", "masked_position", "speech_mask", "text_mask", "speech_segment_pos", "text_segment_pos")})
    assert padded["speech"].shape[1] == 208 and (208 + padded["text"].shape[1]) % 8 == 0
    l32, _, _ = m32(**padded)
    assert abs(float(l16) - float(l32)) < 1e-2 * abs(float(l32)), (float(l16), float(l32))
    assert bool(torch.isfinite(m16.store.grad).all())
    m16.load_state_dict(sd), m32.load_state_dict(sd)
    m16.eval(), m32.eval()
    b1 = {k: v[:1] for k, v in batch.items()}
    with torch.no_grad():
        o16 = m16.inference(**b1, span_boundary=[40, 90], use_teacher_forcing=True)["feat_gen"]
        o32 = m32.inference(**b1, span_boundary=[40, 90], use_teacher_forcing=True)["feat_gen"]
    assert o16[0].shape == o32[0].shape and o16[2].shape == o32[2].shape == (1, 203 - 90, oc.odim)
    np.testing.assert_allclose(o16[1].float().cpu().numpy(), o32[1].cpu().numpy(), atol=0.15, rtol=5e-2)


def test_training_makes_progress_and_bf16_tracks_fp32_trajectory():
    """30 optimizer steps (clip + Adam + Noam on the flat buffers) on a fixed batch: the masked-L1 loss must fall
    substantially and the bf16 trajectory must stay close to the fp32 one (dropout off so both see the same function)."""
    from a3t_amd.config import A3TConfig
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    from a3t_amd.trainer import A3TTrainer
    from a3t_amd.collate import synthetic_batch
    c = A3TConfig(adim=128, heads=2, ff=256, enc_blocks=2, dec_blocks=2, postnet_layers=3, postnet_chans=64, vocab=40)
    batch = synthetic_batch(c, 4, 192, 32, seed=7, device=DEV)
    traj = {}
    for compute in ("f32", "bf16"):
        store = ParamStore(c, DEV)
        xavier_init_(store, seed=3, bn_gamma=1.0)
        tr = A3TTrainer(c, store, compute=compute, lr=1.0, warmup_steps=20, grad_clip=1.0, dropout=False)
        traj[compute] = [float(tr.step(batch)) for _ in range(30)]
    f, b = traj["f32"], traj["bf16"]
    assert f[-1] < 0.6 * f[0] and b[-1] < 0.6 * b[0], (f[0], f[-1], b[0], b[-1])
    assert all(math.isfinite(v) for v in f + b)
    assert abs(b[0] - f[0]) < 1e-2 * f[0]
    assert abs(b[-1] - f[-1]) < 0.1 * f[-1], (f[-1], b[-1])


def test_engine_vs_oracle_randomised_architectures():
    """8 random small architectures (heads 1/2/4, conv-module kernels 3..31, 1-2 + 1-2 blocks, postnet 2-5 layers) on
    ragged batches: loss, outputs and EVERY parameter gradient of the fp32 HIP engine against the CPU oracle
    (tests/fuzz_engine.py; `python tests/fuzz_engine.py <seed> <cases>` runs longer sweeps)."""
    import fuzz_engine as mod
    assert mod.run(seed=4, n=8, verbose=False) == 0


def test_bf16_schedule_vs_fp32_engine_randomised_architectures():
    """6 random mid-size architectures with the recipe's dropout ON (same counter-RNG masks in both engines): the
    bf16 production schedule must track the exact-fp32 engine (loss 1.5e-2 relative, flat-gradient cosine > 0.98)."""
    import fuzz_engine as mod
    assert mod.run_bf16(seed=2, n=6, verbose=False) == 0


@pytest.mark.parametrize("B,Tf", [(1, 3), (3, 17), (2, 61)])
def test_parallel_wavegan_fused_block_equals_layerwise_path(B, Tf):
    """pwg_fused.hip against the layer-by-layer GEMM path on random weights / lengths (T_wav = 300 * Tf is not a multiple
    of the 256-sample tile; dilations 1..512 reach across tiles and past the utterance ends)."""
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    cfg = O.PWGConfig()
    state = O.procedural_state(O.pwg_param_shapes(cfg), seed=40 + Tf)
    for k in state:
        if "up_layers" in k:
            state[k] = np.abs(state[k]) / np.abs(state[k]).sum()
    rs = np.random.RandomState(Tf)
    c = torch.from_numpy((rs.standard_normal((B, Tf, 80)) * 1.5 - 4.0).astype(np.float32))
    z = torch.from_numpy(rs.standard_normal((B, Tf * 300, 1)).astype(np.float32))
    a = ParallelWaveGANGeneratorHIP(state, device=DEV, fused=True).inference(c, z)
    b = ParallelWaveGANGeneratorHIP(state, device=DEV, fused=False).inference(c, z)
    assert a.shape == (B, Tf * 300, 1)
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=2e-5, rtol=1e-4)
    # the batched upsampling network (replication pad, stretch + smoothing per utterance) against every utterance run on
    # its own, and against the oracle's generator for the last one
    voc = ParallelWaveGANGeneratorHIP(state, device=DEV, fused=True)
    for i in range(B):
        one = voc.inference(c[i], z[i])
        np.testing.assert_allclose(a[i].cpu().numpy(), one.cpu().numpy(), atol=1e-6, rtol=1e-5)
    with torch.no_grad():
        ref = O.pwg_forward(O.to_torch_state(state), c[B - 1].t()[None], z[B - 1].t()[None], cfg)   # (B, 80, T), (B, 1, T_wav)
    np.testing.assert_allclose(a[B - 1].cpu().numpy(), ref.numpy().reshape(-1, 1), atol=5e-5, rtol=1e-4)


@pytest.mark.parametrize("kind", ["replace", "mask", "append", "delete"])
def test_speech_editor_end_to_end_against_oracle(kind):
    """The speech-editing driver on the device path (a3t_amd.sedit.SpeechEditor: plan on the host -> log-mel collate on
    the GPU -> teacher-forced Conformer infill -> fused ParallelWaveGAN -> splice into the original audio) against the
    oracle's restatement of the same chain (span arithmetic pinned by the reference driver's own outputs in
    tests/golden/sedit.json; collate / infill / vocoder pinned by their goldens), on an edit taken from that fixture."""
    import json
    import sys
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    from a3t_amd.sedit import SpeechEditor
    from a3t_amd.task import MLMTask
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden import fake_phone_duration
    fx = json.load(open(os.path.join(G, "sedit.json")))
    case = [c for c in fx["cases"] if c["kind"] == kind][0]
    rs = np.random.RandomState(5)
    wav = np.load(os.path.join(G, "sedit_wav.npz"))[case["wav"] + ".in"]
    wav = (0.1 * rs.standard_normal(wav.shape[0])).astype(np.float32)            # a signal with a spectrum
    oc = O.tiny_config()
    model = MLMTask.build_model(_task_args(oc), device=DEV)
    state = O.procedural_state(O.param_shapes(oc), 1)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    fe = LogMelFbank(fs=oc.fs, n_fft=oc.n_fft, win_length=oc.win_length, hop_length=oc.hop_length, n_mels=oc.n_mels,
                     fmin=oc.fmin, fmax=oc.fmax, device=DEV)
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob, mean_phn_span=oc.mean_phn_span,
                        sega_emb=True)
    cfg = O.PWGConfig()
    vstate = O.procedural_state(O.pwg_param_shapes(cfg), seed=4)
    for k in vstate:
        if "up_layers" in k:
            vstate[k] = np.abs(vstate[k]) / np.abs(vstate[k]).sum()
    voc = ParallelWaveGANGeneratorHIP(vstate, device=DEV)
    noise = {}

    def vocoder(feat):
        noise["z"] = torch.from_numpy(np.random.RandomState(9).standard_normal((feat.shape[0] * oc.hop_length, 1)).astype(np.float32))
        return voc.inference(feat, noise["z"])

    ids = lambda phns: np.array([2 + sum(map(ord, ph)) % (oc.vocab - 4) for ph in phns], dtype=np.int64)
    ed = SpeechEditor(model, coll, vocoder, ids, fake_phone_duration)
    args = (case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"], case["old_str"], case["new_str"])
    got = ed.edit(wav, *args, **case["opts"])

    # ---- the same chain through the oracle
    ms, me, op, nph, rep, add = O.sedit_phone_spans(*args)
    nwav, phns, ns, ne, ob, nb = O.sedit_plan_edit(wav, oc.fs, oc.hop_length, ms, me, op, nph, rep, add, fake_phone_duration,
                                                   case["new_str"], **case["opts"])
    assert got["old_span_boundary"] == ob and got["new_span_boundary"] == nb
    data = [("1", dict(speech=np.asarray(nwav, np.float32), align_start=np.asarray(ns), align_end=np.asarray(ne),
                       text=ids(phns), span_boundary=np.asarray(nb)))]
    _, b = O.collate(data, oc)
    p = O.to_torch_state(state)
    feat = O.inference_splice(p, b, oc, (nb[0], nb[1]))
    assert got["feat"].shape == feat.shape
    np.testing.assert_allclose(got["feat"].cpu().numpy(), feat.numpy(), atol=1e-3, rtol=1e-3)
    pv = O.to_torch_state(vstate)
    ref_wav = O.pwg_forward(pv, feat.t()[None], noise["z"].t()[None], cfg)[0, 0].numpy()
    assert got["prediction"].shape == ref_wav.shape == (feat.shape[0] * oc.hop_length,)
    np.testing.assert_allclose(got["prediction"], ref_wav, atol=2e-3 * max(1.0, float(np.abs(ref_wav).max())), rtol=0)
    ref_edit = O.sedit_replace_waveform(wav, ref_wav, oc.hop_length, ob, nb)
    assert got["orgin_replaced"].shape == ref_edit.shape
    np.testing.assert_allclose(got["orgin_replaced"], ref_edit, atol=2e-3 * max(1.0, float(np.abs(ref_wav).max())), rtol=0)
    # outside the edited span the result IS the input audio
    h = oc.hop_length
    assert np.array_equal(got["orgin_replaced"][:h * ob[0]], wav[:h * ob[0]])
    if h * ob[1] < len(wav):
        assert np.array_equal(got["orgin_replaced"][h * nb[1]:], wav[h * ob[1]:])


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """`bench.py` without --full times the step and reports nothing else; --dump-outputs writes what the last timed step
    computed (loss, mel outputs, sampled parameter / gradient / Adam buffers) as float32 .npy files under 64 MB."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--blocks", "1", "--batch", "4", "--tmel",
                        "200", "--tphn", "24", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["roofline"] is None
    assert not {"comm", "vocoder", "c4", "collate", "cpu_baseline"} & set(out)
    got = {p.stem: np.load(p) for p in d.glob("*.npy")}
    assert set(got) == {"loss", "mel_before", "mel_after", "params", "grad", "adam_m", "adam_v"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(p.stat().st_size for p in d.glob("*.npy")) < 64 << 20
    assert float(got["loss"][0]) == out["config"]["final_loss"]
    assert got["mel_before"].shape == got["mel_after"].shape == (4, 200, 80)
    assert got["params"].shape == got["grad"].shape == (1 << 20,) and np.abs(got["grad"]).max() > 0
