"""Generate tests/golden/hifigan.{npz,json}: the HiFi-GAN generator run by the REFERENCE itself
(espnet2/gan_tts/hifigan/hifigan.py::HiFiGANGenerator, imported through make_golden.install_stubs()), in the build container only.

    python tests/golden/make_golden_hifigan.py

Weights are procedural (tests/hifigan_ref.py::procedural_hifigan_state on oracle.procedural_state) and inputs come from seeds
(hifigan_ref.mel_input); neither is stored.  Stored are the reference's fp64 outputs and, in the JSON, the fp32-vs-fp64 floor F
of every case (max |fp32 - fp64| / scale) that the tests take their bounds from, and the per-stage RMS of the fp64 run.

The generator asserts that the fixture is not vacuous: every stage's output RMS lies in [0.05, 20], fewer than 1 % of the
output samples have |y| > 0.99, two different mels give outputs >= 0.1 of scale apart -- and that the restatement
hifigan_ref.generator agrees with the reference in fp64 to 1e-12."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import hifigan_ref as R                                                                # noqa: E402


def build(cfg, state, weight_norm):
    import torch
    from espnet2.gan_tts.hifigan.hifigan import HiFiGANGenerator
    kw = {k: v for k, v in cfg.items() if k != "negative_slope"}
    m = HiFiGANGenerator(nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": cfg["negative_slope"]},
                         use_weight_norm=weight_norm, **kw)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    return m.eval()


def run(model, mel):
    """(output [T*hop][1], RMS after the input convolution, every stage and the output) of one mel [T][80]."""
    import torch
    with torch.no_grad():
        c = torch.as_tensor(mel).to(next(model.parameters()).dtype).t()[None]
        rms = []
        x = model.input_conv(c)
        rms.append(float(x.double().pow(2).mean().sqrt()))
        for i in range(model.num_upsamples):
            x = model.upsamples[i](x)
            cs = 0.0
            for j in range(model.num_blocks):
                cs += model.blocks[i * model.num_blocks + j](x)
            x = cs / model.num_blocks
            rms.append(float(x.double().pow(2).mean().sqrt()))
        x = model.output_conv(x)
        rms.append(float(x.double().pow(2).mean().sqrt()))
        y = model.inference(torch.as_tensor(mel).to(x.dtype))
        assert torch.equal(y, x[0].t())
    return y.numpy(), rms


def main():
    import make_golden
    make_golden.install_stubs()
    import torch
    torch.set_num_threads(1)
    arrays, meta = {}, dict(frames=list(R.FRAMES), cases={})
    for name, case in R.CASES.items():
        cfg, seed, wn = case["cfg"], case["seed"], case["weight_norm"]
        state = R.procedural_hifigan_state(cfg, seed, wn)
        model = build(cfg, state, wn)
        m64 = build(cfg, state, wn).double()      # (a weight-normed module cannot be deep-copied after a forward)
        info = dict(cfg=cfg, seed=seed, weight_norm=wn, hop=R.hop_of(cfg), F={}, rms={}, saturated={})
        for T in R.FRAMES:
            mel = R.mel_input(T, seed)
            y32, _ = run(model, mel)
            y64, rms = run(m64, mel.astype(np.float64))
            assert y64.shape == (T * R.hop_of(cfg), 1)
            assert all(0.05 <= v <= 20.0 for v in rms), (name, T, rms)
            sat = float((np.abs(y64) > 0.99).mean())
            assert sat < 0.01, (name, T, sat)
            mine = R.generator(state, cfg, torch.from_numpy(mel), dtype=torch.float64).numpy()
            assert np.abs(mine - y64).max() <= 1e-12, (name, T, np.abs(mine - y64).max())
            arrays[f"{name}.T{T}.wav64"] = y64
            info["F"][str(T)] = float(np.abs(y32.astype(np.float64) - y64).max() / R.scale_of(y64))
            info["rms"][str(T)] = [round(v, 4) for v in rms]
            info["saturated"][str(T)] = sat
            print(name, "T", T, "F", info["F"][str(T)], "rms", info["rms"][str(T)], "saturated", sat)
        T = max(R.FRAMES)
        other, _ = run(m64, R.mel_input(T, seed + 100).astype(np.float64))
        apart = float(np.abs(other - arrays[f"{name}.T{T}.wav64"]).max() / R.scale_of(other))
        assert apart >= 0.1, (name, apart)
        info["mels_apart"] = apart
        print(name, "two mels apart", apart)
        meta["cases"][name] = info
    np.savez_compressed(os.path.join(HERE, "hifigan.npz"), **arrays)
    with open(os.path.join(HERE, "hifigan.json"), "w") as f:
        json.dump(meta, f, indent=1)
    for n in ("hifigan.npz", "hifigan.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
