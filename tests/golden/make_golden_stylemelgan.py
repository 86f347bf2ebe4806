"""Generate tests/golden/stylemelgan.{npz,json}: the StyleMelGAN generator run by the REFERENCE itself
(espnet2/gan_tts/style_melgan/style_melgan.py::StyleMelGANGenerator.inference, imported through make_golden.install_stubs()), in
the build container only.

    python tests/golden/make_golden_stylemelgan.py

scipy.signal.kaiser, which the reference's package imports (PQMF), left scipy: the script sets it to scipy.signal.windows.kaiser
before the import.  The reference's inference draws its noise with torch.randn; the script hands it the seeded noise of
stylemelgan_ref.noise_input there (in the model's dtype: the reference's own float32 noise does not enter its .double() model).
Weights are procedural (stylemelgan_ref.procedural_stylemelgan_state on oracle.procedural_state) and inputs come from seeds
(stylemelgan_ref.mel_input / noise_input); neither is stored.  Stored are the reference's fp64 waveforms and, in the JSON, the
seeds, the fp32-vs-fp64 floor F of every case (max |fp32 - fp64| / scale) that the tests take their bounds from and the RMS of
every block's output in the fp64 run.

The generator asserts that the fixture is not vacuous: F <= 2e-5 in every case (if it fails, lower the case's gate_gain, not the
cap), every block's RMS lies in [0.02, 20], no sample has |y| > 0.99, at each case's longest input two different z give outputs
>= 0.1 of scale apart -- and that the restatement stylemelgan_ref.generator agrees with the reference in fp64 to 1e-12."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import stylemelgan_ref as R                                                           # noqa: E402


def build(cfg, state, weight_norm):
    import torch
    from espnet2.gan_tts.style_melgan.style_melgan import StyleMelGANGenerator
    kw = {k: v for k, v in cfg.items() if k != "noise_upsample_negative_slope"}
    m = StyleMelGANGenerator(noise_upsample_activation="LeakyReLU",
                             noise_upsample_activation_params={"negative_slope": cfg["noise_upsample_negative_slope"]},
                             upsample_mode="nearest", use_weight_norm=weight_norm, **kw)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    return m.eval()


def run(model, mel, z):
    """(waveform [T*hop][1], RMS of every block's output) of one mel [T][aux] with the noise z [m][in]."""
    import torch
    dt = next(model.parameters()).dtype
    rms, hooks = [], []
    for blk in model.blocks:
        hooks.append(blk.register_forward_hook(lambda m, i, o: rms.append(float(o[0].double().pow(2).mean().sqrt()))))
    zt = torch.as_tensor(z).to(dt).t()[None]
    randn = torch.randn

    def seeded(*size, **kw):
        assert tuple(size) == tuple(zt.shape), (size, zt.shape)
        return zt

    torch.randn = seeded
    try:
        with torch.no_grad():
            y = model.inference(torch.as_tensor(mel).to(dt))
    finally:
        torch.randn = randn
        for h in hooks:
            h.remove()
    return y.numpy(), rms


def main():
    import make_golden
    make_golden.install_stubs()
    import scipy.signal
    import scipy.signal.windows
    scipy.signal.kaiser = scipy.signal.windows.kaiser
    import torch
    torch.set_num_threads(1)
    arrays, meta = {}, dict(cases={})
    for name, case in R.CASES.items():
        cfg, seed, wn = case["cfg"], case["seed"], case["weight_norm"]
        state = R.case_state(name)
        model = build(cfg, state, wn)
        m64 = build(cfg, state, wn).double()      # (a weight-normed module cannot be deep-copied after a forward)
        hop = R.hop_of(cfg)
        info = dict(cfg=cfg, seed=seed, mel_seed=1000 + seed, noise_seed=2000 + seed,      # (the RandomState seeds of mel_input / noise_input)
                    weight_norm=wn, gate_gain=case["gate_gain"], hop=hop, noise_factor=R.noise_factor(cfg),
                    frames=list(case["frames"]), F={}, rms={})
        for T in case["frames"]:
            mel, z = R.mel_input(T, seed, cfg["aux_channels"]), R.noise_input(cfg, T, seed)
            y32, _ = run(model, mel, z)
            y64, rms = run(m64, mel.astype(np.float64), z.astype(np.float64))
            assert y64.shape == (T * hop, 1)
            assert all(0.02 <= v <= 20.0 for v in rms), (name, T, rms)
            assert np.abs(y64).max() <= 0.99, (name, T, np.abs(y64).max())
            mine = R.generator(state, cfg, torch.from_numpy(mel), torch.from_numpy(z), dtype=torch.float64).numpy()
            assert np.abs(mine - y64).max() <= 1e-12, (name, T, np.abs(mine - y64).max())
            Fl = float(np.abs(y32.astype(np.float64) - y64).max() / R.scale_of(y64))
            assert Fl <= 2e-5, (name, T, Fl)
            arrays[f"{name}.T{T}.wav64"] = y64
            info["F"][str(T)] = Fl
            info["rms"][str(T)] = [round(v, 4) for v in rms]
            print(name, "T", T, "F", Fl, "rms", info["rms"][str(T)], "max", float(np.abs(y64).max()))
        T = max(case["frames"])
        other, _ = run(m64, R.mel_input(T, seed, cfg["aux_channels"]).astype(np.float64),
                       R.noise_input(cfg, T, seed + 100).astype(np.float64))
        apart = float(np.abs(other - arrays[f"{name}.T{T}.wav64"]).max() / R.scale_of(other))
        assert apart >= 0.1, (name, apart)
        info["noises_apart"] = apart
        print(name, "two noises apart", apart)
        meta["cases"][name] = info
    np.savez_compressed(os.path.join(HERE, "stylemelgan.npz"), **arrays)
    with open(os.path.join(HERE, "stylemelgan.json"), "w") as f:
        json.dump(meta, f, indent=1)
    total = 0
    for n in ("stylemelgan.npz", "stylemelgan.json"):
        total += os.path.getsize(os.path.join(HERE, n))
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")
    assert total < 512 * 1024, total


if __name__ == "__main__":
    main()
