"""Generate tests/golden/mlm_transformer.npz / .json by running the REFERENCE model itself with `encoder: transformer`
(MLMEncoder / MLMDecoder of transformer/encoder.py:370-777; build container only, like make_golden.py):

    python tests/golden/make_golden_mlm_transformer.py

  a  input_layer sega_mlm, PositionalEncoding, positionwise_layer_type linear, decoder transformer
  b  use_scaled_pos_enc (speech alpha 1.3, text alpha 0.7), conv1d k = 3, 2 encoder blocks, decoder transformer
  c  input_layer mlm, decoder no_decoder

All at oracle.tiny_config() (adim 32, 2 heads), procedural weights over the variant's own key set, every dropout probability 0,
the batch of mlm_variants.  Only the seeds and the reference's numeric outputs are stored: mlm_transformer.npz (losses, outputs,
the inference splice, and `<case>.err.<output>` = the largest absolute distance of the reference's own fp32 run from its fp64 run over
that output's elements), mlm_transformer_grads_{a,b,c}.npz (every parameter gradient) and mlm_transformer.json
(options, key names and shapes).
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
from make_golden_mlm_variants import BATCH_KEYS, SEED_B, SEED_W  # noqa: E402

CASES = {
    "a": dict(input_layer="sega_mlm", positionwise_layer_type="linear", positionwise_conv_kernel_size=1, enc_blocks=1,
              use_scaled_pos_enc=False, decoder="transformer"),
    "b": dict(input_layer="sega_mlm", positionwise_layer_type="conv1d", positionwise_conv_kernel_size=3, enc_blocks=2,
              use_scaled_pos_enc=True, decoder="transformer"),
    "c": dict(input_layer="mlm", positionwise_layer_type="linear", positionwise_conv_kernel_size=1, enc_blocks=1,
              use_scaled_pos_enc=False, decoder="no_decoder"),
}
ALPHAS = {"encoder.speech_embed.4.alpha": 1.3, "encoder.text_embed.1.alpha": 0.7}


def confs(c, opt):
    """(encoder_conf, decoder_conf) of one case, as a recipe yaml would spell them."""
    enc = dict(attention_dim=c.adim, attention_heads=c.heads, linear_units=c.ff, num_blocks=opt["enc_blocks"],
               dropout_rate=0.2, positional_dropout_rate=0.2, attention_dropout_rate=0.2, input_layer=opt["input_layer"],
               normalize_before=True, concat_after=False, positionwise_layer_type=opt["positionwise_layer_type"],
               positionwise_conv_kernel_size=opt["positionwise_conv_kernel_size"], selfattention_layer_type="selfattn",
               pre_speech_layer=0)
    dec = dict(attention_dim=c.adim, attention_heads=c.heads, linear_units=c.ff, num_blocks=c.dec_blocks, dropout_rate=0.2,
               positional_dropout_rate=0.2, attention_dropout_rate=0.2, normalize_before=True, concat_after=False,
               positionwise_layer_type=opt["positionwise_layer_type"],
               positionwise_conv_kernel_size=opt["positionwise_conv_kernel_size"], selfattention_layer_type="selfattn")
    return enc, dec


def build_variant(c, vocab, opt):
    import yaml
    from argparse import Namespace
    from espnet2.tasks.mlm import MLMTask

    conf = yaml.safe_load(open(os.path.join(MG.REF, "egs2/vctk/sedit/conf/fsp2_conformer.yaml")))
    mc = copy.deepcopy(conf["model_conf"])
    mc.update(postnet_layers=c.postnet_layers, postnet_chans=c.postnet_chans, postnet_filts=c.postnet_filts,
              mlm_prob=c.mlm_prob, mean_phn_span=c.mean_phn_span)
    enc, dec = confs(c, opt)
    fconf = dict(n_fft=c.n_fft, hop_length=c.hop_length, win_length=c.win_length, fs=c.fs, fmin=c.fmin, fmax=c.fmax,
                 n_mels=c.n_mels)
    args = Namespace(token_list=(["<blank>", "<unk>", "<space>"] + [f"t{i}" for i in range(vocab - 4)] + ["<sos/eos>"]),
                     odim=c.odim, input_size=c.idim, feats_extract="fbank", feats_extract_conf=fconf, normalize=None,
                     normalize_conf={}, use_scaled_pos_enc=opt["use_scaled_pos_enc"], encoder="transformer", encoder_conf=enc,
                     decoder=opt["decoder"], decoder_conf=dec, model_conf=mc, init=conf["init"])
    return MLMTask.build_model(args)


def load_procedural(model, seed):
    import torch
    from oracle.a3t_oracle import procedural_state

    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    state = procedural_state(shapes, seed)
    for k, a in ALPHAS.items():
        if k in state:
            state[k] = np.array(a, dtype=np.float32)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return shapes


def run_case(model, batch, c):
    """loss, before, after, gradients (training mode), eval loss and the inference splice of one model at its dtype."""
    import torch
    fw = dict(speech_pad=batch["speech"], text_pad=batch["text"], masked_position=batch["masked_position"],
              speech_mask=batch["speech_mask"], text_mask=batch["text_mask"],
              speech_segment_pos=batch["speech_segment_pos"], text_segment_pos=batch["text_segment_pos"])
    load_procedural(model, SEED_W)
    model.train()
    before, after, _, _ = model._forward(fw, batch["speech_segment_pos"])
    load_procedural(model, SEED_W)      # reset the postnet's BatchNorm statistics the probe forward touched
    model.train()
    model.zero_grad()
    loss, _ = MG.run_model(model, batch)
    loss.backward()
    r = dict(loss=loss.detach().numpy(), before=before.detach().numpy(), after=after.detach().numpy())
    for n, p in model.named_parameters():
        assert p.grad is not None, n
        r["grad." + n] = p.grad.numpy().copy()
    load_procedural(model, SEED_W)
    model.eval()
    with torch.no_grad():
        loss_e, _ = MG.run_model(model, batch)
        inf = model.inference(**{k: batch[k][:1] for k in BATCH_KEYS}, span_boundary=[10, 30], use_teacher_forcing=True)
    r["loss_eval"] = loss_e.numpy()
    r["infer_splice"] = torch.cat([inf["feat_gen"][0][0], inf["feat_gen"][1], inf["feat_gen"][2][0]], dim=0).numpy()
    return r


def main(out):
    import torch
    from oracle.a3t_oracle import synthetic_batch, tiny_config

    MG.install_stubs()
    c = tiny_config()
    d, meta = {}, {}
    for tag, opt in CASES.items():
        model = build_variant(c, c.vocab, opt)
        shapes = load_procedural(model, SEED_W)
        batch = synthetic_batch(c, B=2, T_mel=48, T_phn=8, seed=SEED_B, lengths=[48, 37], text_lengths=[8, 6])
        if opt["input_layer"] == "mlm":        # what the reference's collate hands a model without segment embedding
            batch["speech_segment_pos"].zero_()
            batch["text_segment_pos"].zero_()
        r = run_case(model, batch, c)
        # the reference's own rounding: the same model and batch in fp64
        m64 = build_variant(c, c.vocab, opt).double()
        b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
        r64 = run_case(m64, b64, c)
        for k, v in r.items():
            ref = np.asarray(r64[k], dtype=np.float64)
            d[f"{tag}.err.{k}"] = np.array(float(np.abs(np.asarray(v, dtype=np.float64) - ref).max()))
            d[f"{tag}.{k}"] = v
        meta[tag] = dict(options=opt, keys={k: list(s) for k, s in shapes.items()})
        print(tag, opt, "keys", len(shapes), "loss", float(r["loss"].reshape(-1)[0]), "eval", float(r["loss_eval"].reshape(-1)[0]), "worst fp32 distance",
              max((float(v), k) for k, v in d.items() if k.startswith(tag + ".err.")))
    np.savez_compressed(os.path.join(out, "mlm_transformer.npz"), **{k: v for k, v in d.items() if ".grad." not in k or ".err." in k})
    for tag in CASES:
        np.savez_compressed(os.path.join(out, f"mlm_transformer_grads_{tag}.npz"),
                            **{k: v for k, v in d.items() if k.startswith(tag + ".grad.")})
    with open(os.path.join(out, "mlm_transformer.json"), "w") as fh:
        json.dump(dict(seed_weights=SEED_W, seed_batch=SEED_B, alphas=ALPHAS, cases=meta), fh, indent=0, sort_keys=True)


if __name__ == "__main__":
    main(HERE)
