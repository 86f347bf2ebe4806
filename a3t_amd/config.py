"""Hyper-parameters of the A3T masked-mel model (host-side mirror of what
MLMTask.build_model reads from the recipe yaml: espnet2/tasks/mlm.py:328-443,
egs2/vctk/sedit/conf/fsp2_conformer.yaml:27-75)."""
from dataclasses import dataclass
from typing import Any, Dict


@dataclass
class A3TConfig:
    idim: int = 80
    odim: int = 80
    vocab: int = 73
    adim: int = 384
    heads: int = 2
    ff: int = 1536
    ff_kernel: int = 3
    enc_blocks: int = 4
    dec_blocks: int = 4
    enc_kernel: int = 7
    dec_kernel: int = 31
    postnet_layers: int = 5
    postnet_chans: int = 256
    postnet_filts: int = 5
    max_len: int = 5000
    seg_table: int = 500
    lsm_weight: float = 0.1
    dropout_rate: float = 0.2
    positional_dropout_rate: float = 0.2
    attention_dropout_rate: float = 0.2
    postnet_dropout_rate: float = 0.5
    # speaker conditioning (BASELINE configs[3] "+ x-vector cond"): spembs (B, spk_embed_dim) -> Linear -> added to every token
    # after the embedding prologue.  The reference accepts `spembs` and ignores it (sedit_model.py:246): this is an
    # extension with no reference behaviour (parity unpinned); 0 = off, the reference's behaviour.
    spk_embed_dim: int = 0
    # model variants the reference's MLMTask builds besides the recipe's (conformer/encoder.py:386-398, :502-516; tasks/mlm.py:405-413)
    segment_emb: bool = True     # input_layer 'sega_mlm'; False = 'mlm': no segment table, segment ids are not read
    pre_blocks: int = 0          # pre_speech_layer: conformer blocks over the speech tokens alone, before the text joins
    has_decoder: bool = True     # False = decoder 'no_decoder': the head reads encoder.after_norm (no sqrt(d) scale, no decoder.after_norm)
    # feature extraction
    fs: int = 24000
    n_fft: int = 2048
    win_length: int = 1200
    hop_length: int = 300
    n_mels: int = 80
    fmin: float = 80.0
    fmax: float = 7600.0
    # masking
    mlm_prob: float = 0.8
    mean_phn_span: int = 8

    @property
    def dk(self) -> int:
        return self.adim // self.heads

    @staticmethod
    def from_espnet(encoder_conf: Dict[str, Any], decoder_conf: Dict[str, Any], model_conf: Dict[str, Any],
                    input_size: int, odim: int, vocab: int, feats_conf: Dict[str, Any] = None,
                    has_decoder: bool = True) -> "A3TConfig":
        """Translate the recipe's encoder_conf/decoder_conf/model_conf dictionaries.  has_decoder=False (decoder: no_decoder):
        decoder_conf is not read."""
        e, m = encoder_conf, model_conf
        d = decoder_conf if has_decoder else {}          # (left alone without a decoder, tasks/mlm.py:393-395)
        input_layer = e.get("input_layer", "sega_mlm")
        if input_layer not in ("sega_mlm", "mlm"):
            raise NotImplementedError(f"input_layer={input_layer!r}: only 'sega_mlm' (the A3T recipe) and 'mlm' are implemented")
        pre_blocks = int(e.get("pre_speech_layer", 0) or 0)
        if pre_blocks < 0:
            raise ValueError(f"pre_speech_layer={pre_blocks}: expected 0 or more")
        for conf, who in ((e, "encoder_conf"), (d, "decoder_conf")):
            if conf.get("positionwise_layer_type", "conv1d") != "conv1d":
                raise NotImplementedError(f"{who}.positionwise_layer_type={conf['positionwise_layer_type']!r}: only 'conv1d' "
                                          "(the recipe's MultiLayeredConv1d) is implemented")
            for k in ("macaron_style", "use_cnn_module"):
                if not conf.get(k, True):
                    raise NotImplementedError(f"{who}.{k}=False: only the recipe's conformer block (macaron FFN pair, "
                                              "convolution module) is implemented")
        c = A3TConfig(
            idim=input_size, odim=odim, vocab=vocab, adim=e["attention_dim"], heads=e["attention_heads"],
            ff=e["linear_units"], ff_kernel=e.get("positionwise_conv_kernel_size", 3), enc_blocks=e["num_blocks"],
            dec_blocks=d["num_blocks"] if has_decoder else 0, enc_kernel=e.get("cnn_module_kernel", 31),
            dec_kernel=d.get("cnn_module_kernel", 31), segment_emb=(input_layer == "sega_mlm"), pre_blocks=pre_blocks,
            has_decoder=bool(has_decoder), postnet_layers=m.get("postnet_layers", 0),
            postnet_chans=m.get("postnet_chans", 0), postnet_filts=m.get("postnet_filts", 0),
            lsm_weight=m.get("lsm_weight", 0.0), dropout_rate=e.get("dropout_rate", 0.1),
            positional_dropout_rate=e.get("positional_dropout_rate", 0.1),
            attention_dropout_rate=e.get("attention_dropout_rate", 0.0), mlm_prob=m.get("mlm_prob", 0.25),
            mean_phn_span=m.get("mean_phn_span", 3))
        if feats_conf:
            for k in ("fs", "n_fft", "win_length", "hop_length", "n_mels", "fmin", "fmax"):
                if k in feats_conf and feats_conf[k] is not None:
                    setattr(c, k, feats_conf[k])
        return c


def config_c4(**kw) -> A3TConfig:
    """BASELINE.json configs[3]: LibriTTS multi-speaker, 6 + 6 blocks, d=512, H=4 (d_k=128), ff=2048, x-vector (512-d)
    conditioning."""
    c = A3TConfig(adim=512, heads=4, ff=2048, enc_blocks=6, dec_blocks=6, spk_embed_dim=512)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def config_c2(**kw) -> A3TConfig:
    """BASELINE.json configs[1]: '12-layer' = 6 encoder + 6 decoder blocks, d=384."""
    c = A3TConfig(enc_blocks=6, dec_blocks=6)
    for k, v in kw.items():
        setattr(c, k, v)
    return c
