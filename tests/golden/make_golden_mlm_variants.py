"""Generate tests/golden/mlm_variants.npz / .json by running the REFERENCE model itself for the configurations of
MLMTask.build_model that differ from the recipe's (build container only, like make_golden.py):

    python tests/golden/make_golden_mlm_variants.py

  a  encoder_conf.input_layer: mlm                      (no segment embedding)
  b  encoder_conf.pre_speech_layer: 2                   (conformer blocks over the speech tokens alone)
  c  decoder: no_decoder
  d  mlm + pre_speech_layer: 1 + no_decoder

All at oracle.tiny_config(), procedural weights over the variant's own key set, every dropout probability 0, the batch of
e2e_tiny.npz.  Only inputs' seeds and the reference's numeric outputs are stored: mlm_variants.npz (losses, outputs, BatchNorm buffers,
the inference splice), mlm_variants_grads_{a,b,c,d}.npz (every parameter gradient, one file per case to keep each file
small) and mlm_variants.json (each variant's state-dict key names and shapes).
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

CASES = {
    "a": dict(input_layer="mlm", pre_speech_layer=0, decoder="conformer"),
    "b": dict(input_layer="sega_mlm", pre_speech_layer=2, decoder="conformer"),
    "c": dict(input_layer="sega_mlm", pre_speech_layer=0, decoder="no_decoder"),
    "d": dict(input_layer="mlm", pre_speech_layer=1, decoder="no_decoder"),
}
SEED_W, SEED_B = 1, 11
BATCH_KEYS = ["speech", "text", "masked_position", "speech_mask", "text_mask", "speech_segment_pos", "text_segment_pos"]


def build_variant(c, vocab, input_layer, pre_speech_layer, decoder):
    """make_golden.build_ref_model with the three options passed explicitly."""
    import yaml
    from argparse import Namespace
    from espnet2.tasks.mlm import MLMTask

    conf = yaml.safe_load(open(os.path.join(MG.REF, "egs2/vctk/sedit/conf/fsp2_conformer.yaml")))
    enc = copy.deepcopy(conf["encoder_conf"])
    dec = copy.deepcopy(conf["decoder_conf"])
    mc = copy.deepcopy(conf["model_conf"])
    enc.update(attention_dim=c.adim, attention_heads=c.heads, linear_units=c.ff, num_blocks=c.enc_blocks,
               cnn_module_kernel=c.enc_kernel, input_layer=input_layer, pre_speech_layer=pre_speech_layer)
    dec.update(attention_dim=c.adim, attention_heads=c.heads, linear_units=c.ff, num_blocks=c.dec_blocks,
               cnn_module_kernel=c.dec_kernel)
    mc.update(postnet_layers=c.postnet_layers, postnet_chans=c.postnet_chans, postnet_filts=c.postnet_filts,
              mlm_prob=c.mlm_prob, mean_phn_span=c.mean_phn_span)
    fconf = dict(n_fft=c.n_fft, hop_length=c.hop_length, win_length=c.win_length, fs=c.fs, fmin=c.fmin, fmax=c.fmax,
                 n_mels=c.n_mels)
    args = Namespace(token_list=(["<blank>", "<unk>", "<space>"] + [f"t{i}" for i in range(vocab - 4)] + ["<sos/eos>"]),
                     odim=c.odim, input_size=c.idim, feats_extract="fbank", feats_extract_conf=fconf, normalize=None,
                     normalize_conf={}, use_scaled_pos_enc=False, encoder=conf["encoder"], encoder_conf=enc, decoder=decoder,
                     decoder_conf=dec, model_conf=mc, init=conf["init"])
    return MLMTask.build_model(args)


def load_procedural(model, seed):
    import torch
    from oracle.a3t_oracle import procedural_state

    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    state = procedural_state(shapes, seed)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return shapes


def main(out):
    import torch
    from oracle.a3t_oracle import synthetic_batch, tiny_config

    MG.install_stubs()
    c = tiny_config()
    d, meta = {}, {}
    for tag, opt in CASES.items():
        model = build_variant(c, c.vocab, **opt)
        shapes = load_procedural(model, SEED_W)
        batch = synthetic_batch(c, B=2, T_mel=48, T_phn=8, seed=SEED_B, lengths=[48, 37], text_lengths=[8, 6])
        nonzero_seg = {k: batch[k].clone() for k in ("speech_segment_pos", "text_segment_pos")}
        if opt["input_layer"] == "mlm":        # what the reference's collate hands a model without segment embedding
            batch["speech_segment_pos"].zero_()
            batch["text_segment_pos"].zero_()
        fw = dict(speech_pad=batch["speech"], text_pad=batch["text"], masked_position=batch["masked_position"],
                  speech_mask=batch["speech_mask"], text_mask=batch["text_mask"],
                  speech_segment_pos=batch["speech_segment_pos"], text_segment_pos=batch["text_segment_pos"])
        model.train()
        before, after, _, _ = model._forward(fw, batch["speech_segment_pos"])
        load_procedural(model, SEED_W)      # reset the BatchNorm statistics the probe forward touched
        model.train()
        model.zero_grad()
        loss, weight = MG.run_model(model, batch)
        loss.backward()
        r = dict(loss=loss.detach().numpy(), before=before.detach().numpy(), after=after.detach().numpy())
        for n, p in model.named_parameters():
            assert p.grad is not None, n
            r["grad." + n] = p.grad.numpy().copy()
        for n, b in model.named_buffers():
            if "running" in n or "num_batches" in n:
                r["buf." + n] = b.numpy().copy()
        if tag == "a":      # segment ids are ignored by a model without the table
            load_procedural(model, SEED_W)
            model.train()
            with torch.no_grad():
                l2, _ = MG.run_model(model, dict(batch, **nonzero_seg))
            r["loss_nonzero_seg"] = l2.numpy()
            assert float(l2) == float(loss.detach())
        load_procedural(model, SEED_W)
        model.eval()
        with torch.no_grad():
            loss_e, _ = MG.run_model(model, batch)
            inf = model.inference(**{k: batch[k][:1] for k in BATCH_KEYS}, span_boundary=[10, 30], use_teacher_forcing=True)
        r["loss_eval"] = loss_e.numpy()
        r["infer_splice"] = torch.cat([inf["feat_gen"][0][0], inf["feat_gen"][1], inf["feat_gen"][2][0]], dim=0).numpy()
        for k, v in r.items():
            d[f"{tag}.{k}"] = v
        meta[tag] = dict(options=opt, keys={k: list(s) for k, s in shapes.items()})
        print(tag, opt, "keys", len(shapes), "loss", float(loss), "eval", float(loss_e))
    # (every parameter gradient of four models does not fit one committed file: the gradients go into a file per case)
    np.savez_compressed(os.path.join(out, "mlm_variants.npz"), **{k: v for k, v in d.items() if ".grad." not in k})
    for tag in CASES:
        np.savez_compressed(os.path.join(out, f"mlm_variants_grads_{tag}.npz"),
                            **{k: v for k, v in d.items() if k.startswith(tag + ".grad.")})
    with open(os.path.join(out, "mlm_variants.json"), "w") as fh:
        json.dump(dict(seed_weights=SEED_W, seed_batch=SEED_B, cases=meta), fh, indent=0, sort_keys=True)


if __name__ == "__main__":
    main(HERE)
