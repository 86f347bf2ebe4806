"""Generate tests/golden/fs2_duration.{npz,json}: the conformer FastSpeech2 duration path of the speech-editing driver
(the text encoder, the x-vector integration, the DurationPredictor's inference and sedit_inference.py's duration_predict)
run by the REFERENCE itself, in the build container only.

    python tests/golden/make_golden_fs2.py

The reference is imported through make_golden.install_stubs().  Weights are procedural (oracle.procedural_state, keyed by
the FastSpeech2 state-dict names); the fixture stores the name -> shape list, the seeds and the overrides below, so a test
rebuilds the same checkpoint without the reference.  Only inputs and the reference's numeric outputs are stored.

Overrides (after procedural_state; the recipe's xavier init would zero them, the procedural draw would centre the
log-domain duration on 0, i.e. on 0-1 frames):
  duration_predictor.linear.bias      = LINEAR_BIAS (exp(1.8) - 1 = 5 frames at the centre of the spread)
  duration_predictor.conv.{l}.2.weight = 1 + U(-0.2, 0.2)  (RandomState(GAMMA_SEED + l): LayerNorm gammas)
"""
import importlib.machinery
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

LINEAR_BIAS = 1.8
GAMMA_SEED = 1234
LENGTHS = (2, 7, 33, 130, 301)
HS_LENGTH = 33
FS, HOP = 24000, 300
SPK_SEED = 77

_VOWELS = ["AA", "AE", "AH", "AO", "AW", "AY", "EH", "ER", "EY", "IH", "IY", "OW", "OY", "UH", "UW"]
_CONS = ["B", "CH", "D", "DH", "F", "G", "HH", "JH", "K", "L", "M", "N", "NG", "P", "R", "S", "SH", "T", "TH", "V", "W",
         "Y", "Z", "ZH"]
# ESPnet phone token list layout: <blank> first, <unk> second, <sos/eos> last (eos = len(token_list) - 1)
TOKEN_LIST = ["<blank>", "<unk>"] + sorted([v + s for v in _VOWELS for s in "012"] + _CONS) + [",", ".", "?", "<sos/eos>"]

_LJ = dict(adim=384, aheads=2, elayers=4, eunits=1536, dlayers=1, dunits=256, postnet_layers=1, postnet_chans=64,
           positionwise_layer_type="conv1d", positionwise_conv_kernel_size=3, duration_predictor_layers=2,
           duration_predictor_chans=256, duration_predictor_kernel_size=3, encoder_normalize_before=True,
           decoder_normalize_before=True, encoder_type="conformer", decoder_type="conformer",
           conformer_pos_enc_layer_type="rel_pos", conformer_self_attn_layer_type="rel_selfattn",
           conformer_activation_type="swish", use_macaron_style_in_conformer=True, use_cnn_in_conformer=True,
           conformer_enc_kernel_size=7, conformer_dec_kernel_size=31, pitch_predictor_layers=2, pitch_predictor_chans=64,
           energy_predictor_layers=2, energy_predictor_chans=64)
CASES = {
    "lj": dict(_LJ),
    "lj_xadd": dict(_LJ, spk_embed_dim=512, spk_embed_integration_type="add"),
    "lj_xcat": dict(_LJ, spk_embed_dim=512, spk_embed_integration_type="concat"),
    "small_c384": dict(_LJ, adim=256, aheads=2, elayers=2, eunits=1024, conformer_enc_kernel_size=5,
                       duration_predictor_chans=384),
}
SEEDS = {"lj": 21, "lj_xadd": 22, "lj_xcat": 23, "small_c384": 24}
# phone lists of duration_predict beyond the sedit.json plans: `sp` (-> <blank>) and phones outside TOKEN_LIST (-> <unk>)
EXTRA_LISTS = [["sp", "HH", "AH0", "L", "OW1", "sp"], ["DH", "AX0", "K", "AE1", "T", "sp", "[MASK]"], ["sp"],
               ["W", "ER1", "L", "D", "QQ", "sp", "sp", "AY1"]]
SEDIT_KINDS = ("replace", "mask", "append", "delete")


def _sedit_stubs():
    class _Any:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return True

        def __getattr__(self, k):
            return _Any()

    for n in ["matplotlib", "matplotlib.pylab", "parallel_wavegan", "parallel_wavegan.utils", "ipywidgets", "IPython",
              "IPython.display", "espnet2.tasks.tts", "espnet2.bin.align_english"]:
        m = types.ModuleType(n)
        m.__spec__ = importlib.machinery.ModuleSpec(n, None)
        m.__path__ = []

        def _ga(k):
            if k.startswith("__"):
                raise AttributeError(k)
            return _Any()

        m.__getattr__ = _ga
        sys.modules[n] = m


def build_fs2(conf, seed):
    """The reference FastSpeech2 with procedural weights (+ the overrides); returns (model, {name: shape}) keyed by the
    FastSpeech2 state-dict names (an ESPnet TTS checkpoint prefixes them with 'tts.')."""
    import torch
    from espnet2.tts.fastspeech2.fastspeech2 import FastSpeech2
    from oracle.a3t_oracle import procedural_state

    torch.manual_seed(0)
    model = FastSpeech2(idim=len(TOKEN_LIST), odim=80, **conf)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    state = procedural_state(shapes, seed)
    apply_overrides(state, conf.get("duration_predictor_layers", 2))
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    return model, {k: list(s) for k, s in shapes.items()}


def apply_overrides(state, n_layers):
    """The documented overrides, on a procedural_state dict keyed by the FastSpeech2 state-dict names."""
    state["duration_predictor.linear.bias"] = np.full((1,), LINEAR_BIAS, np.float32)
    for l in range(n_layers):
        k = f"duration_predictor.conv.{l}.2.weight"
        rs = np.random.RandomState(GAMMA_SEED + l)
        state[k] = (1.0 + rs.uniform(-0.2, 0.2, state[k].shape)).astype(np.float32)
    return state


def speaker_vector(dim):
    return np.random.RandomState(SPK_SEED).standard_normal(dim).astype(np.float32)


def token_ids(T, seed):
    """T - 1 random phone ids (never <blank>, <unk> or eos) + eos."""
    rs = np.random.RandomState(1000 + T + seed)
    ids = rs.randint(2, len(TOKEN_LIST) - 1, size=T - 1)
    return np.concatenate([ids, [len(TOKEN_LIST) - 1]]).astype(np.int64)


def run_case(model, ids, spembs):
    import torch
    from espnet.nets.pytorch_backend.nets_utils import make_pad_mask
    tts = model
    text = torch.from_numpy(ids)[None]
    ilens = torch.tensor([ids.shape[0]])
    with torch.no_grad():
        hs, _ = tts.encoder(text, tts._source_mask(ilens))
        if spembs is not None:
            hs = tts._integrate_with_spk_embed(hs, torch.from_numpy(spembs)[None])
        dp = tts.duration_predictor
        x = hs.transpose(1, -1)
        for f in dp.conv:
            x = f(x)
        logd = dp.linear(x.transpose(1, -1)).squeeze(-1)
        expm = logd.exp() - dp.offset
        frames = dp.inference(hs, make_pad_mask(ilens))
    assert torch.equal(frames, torch.clamp(torch.round(expm), min=0).long())
    return hs[0].numpy(), logd[0].numpy(), expm[0].numpy(), frames[0].numpy()


def main():
    import make_golden
    make_golden.install_stubs()
    _sedit_stubs()
    import torch
    import espnet2.bin.sedit_inference as S
    from espnet2.text.token_id_converter import TokenIDConverter
    from oracle import a3t_oracle as O
    torch.use_deterministic_algorithms(False)
    torch.set_num_threads(1)

    arrays, meta = {}, dict(token_list=TOKEN_LIST, lengths=list(LENGTHS), hs_length=HS_LENGTH, fs=FS, hop=HOP,
                            spk_seed=SPK_SEED, offset=1.0,
                            overrides={"duration_predictor.linear.bias": LINEAR_BIAS,
                                       "duration_predictor.conv.{l}.2.weight": f"1 + U(-0.2, 0.2), RandomState({GAMMA_SEED} + l)"},
                            cases={})
    models = {}
    for name, conf in CASES.items():
        model, shapes = build_fs2(conf, SEEDS[name])
        models[name] = model
        spk = speaker_vector(conf["spk_embed_dim"]) if conf.get("spk_embed_dim") else None
        if spk is not None:
            arrays[f"{name}.spembs"] = spk
        meta["cases"][name] = dict(tts_conf=conf, seed=SEEDS[name], shapes=shapes)
        for T in LENGTHS:
            ids = token_ids(T, SEEDS[name])
            hs, logd, expm, frames = run_case(model, ids, spk)
            p = f"{name}.T{T}."
            arrays[p + "ids"], arrays[p + "logd"], arrays[p + "expm1"], arrays[p + "frames"] = ids, logd, expm, frames
            if T == HS_LENGTH:
                arrays[p + "hs"] = hs
            print(name, T, "frames", frames[:12].tolist(), "zeros", int((frames == 0).sum()), "distinct",
                  len(set(frames.tolist())))

    # sedit_inference.duration_predict itself, on the "lj" model (and on "lj_xadd" with its x-vector as `sid`)
    proc = types.SimpleNamespace(token_id_converter=TokenIDConverter(TOKEN_LIST))
    records = []

    def ref_duration(model_name, sid):
        fs2 = types.SimpleNamespace(tts=models[model_name])

        def fn(phns):
            out = S.duration_predict(list(phns), FS, HOP, fs2, proc, None, sid=sid)
            records.append(dict(model=model_name, spembs=sid is not None, phns=list(phns), seconds=out))
            return out
        return fn

    for phns in EXTRA_LISTS:
        ref_duration("lj", None)(phns)
    ref_duration("lj_xadd", arrays["lj_xadd.spembs"])(EXTRA_LISTS[0])
    fx = json.load(open(os.path.join(HERE, "sedit.json")))
    for kind in SEDIT_KINDS:
        case = [c for c in fx["cases"] if c["kind"] == kind][0]
        args = (case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"], case["old_str"], case["new_str"])
        ms, me, op, nph, rep, add = O.sedit_phone_spans(*args)
        wav = np.zeros(int(np.ceil(me[-1] * FS)) + HOP, np.float32)
        O.sedit_plan_edit(wav, FS, HOP, ms, me, op, nph, rep, add, ref_duration("lj", None), case["new_str"], **case["opts"])
    for r in records:
        assert all(isinstance(v, float) for v in r["seconds"])
    meta["duration_predict"] = records
    meta["sedit_kinds"] = list(SEDIT_KINDS)
    np.savez_compressed(os.path.join(HERE, "fs2_duration.npz"), **arrays)
    with open(os.path.join(HERE, "fs2_duration.json"), "w") as f:
        json.dump(meta, f, indent=1)
    for n in ("fs2_duration.npz", "fs2_duration.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
