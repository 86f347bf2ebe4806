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
    # encoder / decoder 'transformer' (transformer/encoder.py:370-777): pre-LN blocks of plain MultiHeadedAttention + position-wise
    # FFN, absolute positions added in the prologue and at the decoder entry.  ff_kernel = 1 is positionwise_layer_type 'linear'.
    block: str = "conformer"     # "conformer" | "transformer"
    scaled_pos: bool = False     # use_scaled_pos_enc: x + alpha * pe with two trained scalars (speech, text); transformer only
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
                    has_decoder: bool = True, block: str = "conformer", scaled_pos: bool = False) -> "A3TConfig":
        """Translate the recipe's encoder_conf/decoder_conf/model_conf dictionaries.  has_decoder=False (decoder: no_decoder):
        decoder_conf is not read.  block="transformer" (encoder: transformer): _from_espnet_transformer."""
        e, m = encoder_conf, model_conf
        d = decoder_conf if has_decoder else {}          # (left alone without a decoder, tasks/mlm.py:393-395)
        input_layer = e.get("input_layer", "sega_mlm")
        if input_layer not in ("sega_mlm", "mlm"):
            raise NotImplementedError(f"input_layer={input_layer!r}: only 'sega_mlm' (the A3T recipe) and 'mlm' are implemented")
        pre_blocks = int(e.get("pre_speech_layer", 0) or 0)
        if pre_blocks < 0:
            raise ValueError(f"pre_speech_layer={pre_blocks}: expected 0 or more")
        if block == "transformer":
            c = A3TConfig._from_espnet_transformer(e, d, m, input_size, odim, vocab, has_decoder, scaled_pos,
                                                   input_layer == "sega_mlm", pre_blocks)
            return A3TConfig._with_feats(c, feats_conf)
        if block != "conformer":
            raise NotImplementedError(f"block={block!r}: expected 'conformer' or 'transformer'")
        if scaled_pos:
            raise NotImplementedError("use_scaled_pos_enc=True: the conformer encoder never builds pos_enc_class "
                                      "(ScaledPositionalEncoding is reachable with encoder: transformer only)")
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
        return A3TConfig._with_feats(c, feats_conf)

    @staticmethod
    def _with_feats(c, feats_conf):
        if feats_conf:
            for k in ("fs", "n_fft", "win_length", "hop_length", "n_mels", "fmin", "fmax"):
                if k in feats_conf and feats_conf[k] is not None:
                    setattr(c, k, feats_conf[k])
        return c

    @staticmethod
    def _from_espnet_transformer(e, d, m, input_size, odim, vocab, has_decoder, scaled_pos, segment_emb, pre_blocks):
        """encoder: transformer with decoder: transformer | no_decoder (MLMEncoder / MLMDecoder, transformer/encoder.py:370-777;
        the defaults are that constructor's).  Everything the engine does not run is refused by its field name."""
        if pre_blocks > 0:
            raise NotImplementedError(f"encoder_conf.pre_speech_layer={pre_blocks}: pre-speech blocks are implemented for the "
                                      "conformer encoder only")
        for conf, who in ((e, "encoder_conf"), (d, "decoder_conf")) if has_decoder else ((e, "encoder_conf"),):
            sa = conf.get("selfattention_layer_type", "selfattn")
            if sa != "selfattn":      # (lightconv*, dynamicconv*, longformer; rel_selfattn builds the same class but is not the name)
                raise NotImplementedError(f"{who}.selfattention_layer_type={sa!r}: only 'selfattn' is implemented for a "
                                          "transformer model")
            pw = conf.get("positionwise_layer_type", "linear")
            if pw not in ("linear", "conv1d"):
                raise NotImplementedError(f"{who}.positionwise_layer_type={pw!r}: only 'linear' and 'conv1d' are implemented")
            k = int(conf.get("positionwise_conv_kernel_size", 1)) if pw == "conv1d" else 1
            if k < 1 or k % 2 == 0:
                raise NotImplementedError(f"{who}.positionwise_conv_kernel_size={k}: expected an odd kernel size")
            if not conf.get("normalize_before", True):
                raise NotImplementedError(f"{who}.normalize_before=False: only pre-LN blocks are implemented")
            if conf.get("concat_after", False):
                raise NotImplementedError(f"{who}.concat_after=True is not implemented")
            if float(conf.get("stochastic_depth_rate", 0.0) or 0.0) > 0.0:
                raise NotImplementedError(f"{who}.stochastic_depth_rate={conf['stochastic_depth_rate']}: layer skipping is not "
                                          "implemented")
            if conf.get("intermediate_layers") is not None:
                raise NotImplementedError(f"{who}.intermediate_layers is not implemented")

        def ffn(conf):
            pw = conf.get("positionwise_layer_type", "linear")
            return int(conf.get("positionwise_conv_kernel_size", 1)) if pw == "conv1d" else 1
        if has_decoder:
            for k, dflt in (("attention_dim", 256), ("attention_heads", 4), ("linear_units", 2048)):
                if d.get(k, dflt) != e.get(k, dflt):
                    raise NotImplementedError(f"decoder_conf.{k}={d.get(k, dflt)} differs from encoder_conf.{k}="
                                              f"{e.get(k, dflt)}: one block size per model")
            if ffn(d) != ffn(e):
                raise NotImplementedError("decoder_conf.positionwise_layer_type / positionwise_conv_kernel_size differ from "
                                          "encoder_conf's: one FFN kernel size per model")
        return A3TConfig(
            idim=input_size, odim=odim, vocab=vocab, adim=e.get("attention_dim", 256), heads=e.get("attention_heads", 4),
            ff=e.get("linear_units", 2048), ff_kernel=ffn(e), enc_blocks=e.get("num_blocks", 6),
            dec_blocks=d.get("num_blocks", 6) if has_decoder else 0, segment_emb=segment_emb, pre_blocks=0,
            has_decoder=bool(has_decoder), block="transformer", scaled_pos=bool(scaled_pos),
            postnet_layers=m.get("postnet_layers", 0), postnet_chans=m.get("postnet_chans", 0),
            postnet_filts=m.get("postnet_filts", 0), lsm_weight=m.get("lsm_weight", 0.0), dropout_rate=e.get("dropout_rate", 0.1),
            positional_dropout_rate=e.get("positional_dropout_rate", 0.1),
            attention_dropout_rate=e.get("attention_dropout_rate", 0.0), mlm_prob=m.get("mlm_prob", 0.25),
            mean_phn_span=m.get("mean_phn_span", 3))


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
