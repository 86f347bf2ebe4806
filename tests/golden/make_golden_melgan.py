"""Generate tests/golden/melgan.{npz,json}: the MelGAN / multi-band MelGAN generator run by the REFERENCE itself
(espnet2/gan_tts/melgan/melgan.py::MelGANGenerator and pqmf.py::PQMF, imported through make_golden.install_stubs()), in the build
container only.

    python tests/golden/make_golden_melgan.py

scipy.signal.kaiser, which the reference imports, left scipy: the script sets it to scipy.signal.windows.kaiser before the import.
Weights are procedural (tests/melgan_ref.py::procedural_melgan_state on oracle.procedural_state) and inputs come from seeds
(melgan_ref.mel_input); neither is stored.  Stored are the reference's fp64 waveforms, its fp32 synthesis filters and, in the
JSON, the fp32-vs-fp64 floor F of every case (max |fp32 - fp64| / scale) that the tests take their bounds from, the per-stage
RMS of the fp64 run, the saturated share of the sub-band samples and min_frames (the reference accepts it and rejects one less).

The generator asserts that the fixture is not vacuous: every stage's RMS lies in [0.05, 20], fewer than 1 % of the sub-band
samples have |y| > 0.99, two different mels give outputs >= 0.1 of scale apart, F <= 1e-5 in every case -- and that the
restatement melgan_ref.generator agrees with the reference in fp64 to 1e-12."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import melgan_ref as R                                                                # noqa: E402


def build(cfg, pq, state, weight_norm):
    import torch
    from espnet2.gan_tts.melgan.melgan import MelGANGenerator
    from espnet2.gan_tts.melgan.pqmf import PQMF
    kw = {k: v for k, v in cfg.items() if k != "negative_slope"}
    m = MelGANGenerator(nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": cfg["negative_slope"]},
                        use_weight_norm=weight_norm, **kw)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    return m.eval(), (PQMF(cfg["out_channels"], **pq) if cfg["out_channels"] > 1 else None)


def run(model, pqmf, cfg, mel):
    """(waveform [T*hop][1], sub-band output [T*rate][out_channels], RMS after the input convolution, every stage, the output
    convolution and the PQMF) of one mel [T][80]."""
    import torch
    with torch.no_grad():
        c = torch.as_tensor(mel).to(next(model.parameters()).dtype).t()[None]
        layers, rms = list(model.melgan), []
        _, stages, i_out = R.layer_index(cfg)
        ends = [1] + [st[-1] for _, st in stages] + [len(layers) - 1]
        x = c
        for i, layer in enumerate(layers):
            x = layer(x)
            if i in ends:
                rms.append(float(x.double().pow(2).mean().sqrt()))
        sub = model.inference(torch.as_tensor(mel).to(x.dtype))
        assert torch.equal(sub, x[0].t())
        y = sub
        if pqmf is not None:
            y = pqmf.synthesis(x)[0].t()
            rms.append(float(y.double().pow(2).mean().sqrt()))
    return y.numpy(), sub.numpy(), rms


def accepts(model, T):
    import torch
    try:
        with torch.no_grad():
            model.inference(torch.zeros(T, 80, dtype=next(model.parameters()).dtype))
        return True
    except RuntimeError:
        return False


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
        cfg, pq, seed, wn = case["cfg"], case["pqmf"], case["seed"], case["weight_norm"]
        state = R.procedural_melgan_state(cfg, seed, wn)
        model, pqmf = build(cfg, pq, state, wn)
        m64, pqmf64 = build(cfg, pq, state, wn)      # (a weight-normed module cannot be deep-copied after a forward)
        m64 = m64.double()
        if pqmf is not None:
            pqmf64 = pqmf64.double()
            arrays[f"{name}.synthesis_filter"] = pqmf.synthesis_filter[0].numpy()
            assert arrays[f"{name}.synthesis_filter"].dtype == np.float32
        hop = R.hop_of(cfg)
        info = dict(cfg=cfg, pqmf=pq, seed=seed, weight_norm=wn, hop=hop, frames=list(case["frames"]), F={}, rms={}, saturated={})
        mf = min(case["frames"])
        assert accepts(m64, mf) and not accepts(m64, mf - 1), (name, mf)
        info["min_frames"] = mf
        for T in case["frames"]:
            mel = R.mel_input(T, seed)
            y32, _, _ = run(model, pqmf, cfg, mel)
            y64, sub64, rms = run(m64, pqmf64, cfg, mel.astype(np.float64))
            assert y64.shape == (T * hop, 1)
            assert all(0.05 <= v <= 20.0 for v in rms), (name, T, rms)
            sat = float((np.abs(sub64) > 0.99).mean())
            assert sat < 0.01, (name, T, sat)
            mine = R.generator(state, cfg, torch.from_numpy(mel), pqmf=pq, dtype=torch.float64).numpy()
            assert np.abs(mine - y64).max() <= 1e-12, (name, T, np.abs(mine - y64).max())
            Fl = float(np.abs(y32.astype(np.float64) - y64).max() / R.scale_of(y64))
            assert Fl <= 1e-5, (name, T, Fl)
            arrays[f"{name}.T{T}.wav64"] = y64
            info["F"][str(T)] = Fl
            info["rms"][str(T)] = [round(v, 4) for v in rms]
            info["saturated"][str(T)] = sat
            print(name, "T", T, "F", Fl, "rms", info["rms"][str(T)], "saturated", sat)
        T = max(case["frames"])
        other, _, _ = run(m64, pqmf64, cfg, R.mel_input(T, seed + 100).astype(np.float64))
        apart = float(np.abs(other - arrays[f"{name}.T{T}.wav64"]).max() / R.scale_of(other))
        assert apart >= 0.1, (name, apart)
        info["mels_apart"] = apart
        print(name, "min_frames", mf, "two mels apart", apart)
        meta["cases"][name] = info
    np.savez_compressed(os.path.join(HERE, "melgan.npz"), **arrays)
    with open(os.path.join(HERE, "melgan.json"), "w") as f:
        json.dump(meta, f, indent=1)
    for n in ("melgan.npz", "melgan.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
