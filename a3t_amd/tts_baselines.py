"""The mel arithmetic of the speech-editing driver's three TTS baselines (espnet2/bin/sedit_inference.py:160-260): what
get_baseline1 / get_baseline2 / get_baseline3 do with the result of tts_model.inference before the vocoder.  Pure functions
over FS2TTSModel.synthesize's dict and the original utterance's log-mel; each result goes to any vocoder class's inference.

  baseline 1: the whole new sentence synthesised (:177-183);
  baseline 2: the target words alone synthesised, the eos frames cut off with [:-eos_duration] as the reference writes it
              (an eos of 0 frames therefore leaves nothing), spliced over the old span of the original mel (:207-220);
  baseline 3: the whole new sentence synthesised, the frames of the phones span_tobe_added[0]:span_tobe_added[1] -- from
              sum(durations[:a]) to sum(durations[:b]) -- spliced over the old span (:244-258).
The old span's frames are int(mfa_start[i] * fs / hop_length) of the span's two phone indices, in Python floats as there."""
from typing import Dict, List, Sequence

import torch


def output_feat(out: Dict[str, torch.Tensor]) -> torch.Tensor:
    """feat_gen_denorm when the checkpoint normalises, feat_gen otherwise (:178-181)."""
    d = out.get("feat_gen_denorm")
    return d if d is not None else out["feat_gen"]


def old_span_frames(mfa_start: Sequence[float], span_tobe_replaced: Sequence[int], fs: int, hop_length: int) -> List[int]:
    return [int(mfa_start[span_tobe_replaced[0]] * fs / hop_length), int(mfa_start[span_tobe_replaced[1]] * fs / hop_length)]


def _splice(input_feat, target, old_span):
    input_feat = torch.as_tensor(input_feat).to(target.device, target.dtype)
    return torch.cat([input_feat[:old_span[0]], target, input_feat[old_span[1]:]])


def baseline1_mel(out: Dict[str, torch.Tensor]) -> torch.Tensor:
    """`out`: the synthesis of the whole new sentence."""
    return output_feat(out)


def baseline2_mel(out: Dict[str, torch.Tensor], input_feat, mfa_start, span_tobe_replaced, fs: int, hop_length: int):
    """`out`: the synthesis of the target words alone; input_feat [F][n_mels]: the original utterance's log-mel."""
    eos_duration = int(out["duration"][-1])
    return _splice(input_feat, output_feat(out)[:-eos_duration], old_span_frames(mfa_start, span_tobe_replaced, fs, hop_length))


def baseline3_mel(out: Dict[str, torch.Tensor], input_feat, mfa_start, span_tobe_replaced, span_tobe_added, fs: int,
                  hop_length: int):
    """`out`: the synthesis of the whole new sentence; span_tobe_added: phone indices into the new sentence."""
    durations = out["duration"].tolist()[:-1]
    a, b = sum(durations[:span_tobe_added[0]]), sum(durations[:span_tobe_added[1]])
    return _splice(input_feat, output_feat(out)[a:b], old_span_frames(mfa_start, span_tobe_replaced, fs, hop_length))
