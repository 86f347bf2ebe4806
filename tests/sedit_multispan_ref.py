"""Requests with several separate edits for the multi-span speech editor tests, built from the recorded utterances of
tests/golden/sedit.json: words of the old transcript are swapped, inserted or dropped, new words take their phones from the
stub dictionary LEX (none of its words occurs in the fixture's lexicon, so the word diff is what the test states), kept words
the phones the aligner gave them."""
import json
import os
import sys

import numpy as np

G = os.path.join(os.path.dirname(__file__), "golden")
LEX = {"ZEBRA": ["Z", "IY1", "B", "R", "AH0"], "PLUM": ["P", "L", "AH1", "M"], "OWL": ["AW1", "L"],
       "VIOLET": ["V", "AY1", "AH0", "L", "AH0", "T"]}
OPTS = dict(duration_adjust=True, start_end_sp=False, mask_reconstruct=False)
# recorded utterances (index into sedit.json's cases) and what they are used for
LONG = 1          # DOG ON sp SAT QUIETLY MAT TODAY HOME sp, 3.4 s: two edits far apart
SEVEN = 23        # BLUE SAT CAT sp MAT THE FAST MAT sp, 2.2 s: two and three edits
ONE_PHONE = 18    # A DOG A RAN CAT sp MAT: a one-phone word between a replacement and a deletion


def fixture():
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden import fake_phone_duration
    return json.load(open(os.path.join(G, "sedit.json"))), np.load(os.path.join(G, "sedit_wav.npz")), fake_phone_duration


def old_words(case):
    """[(word, phones)] of the recorded utterance without the `sp` entries."""
    return [(k.split("_")[1], v.split()) for k, v in case["word2phns"].items() if k.split("_")[1] != "sp"]


def rewrite(case, swap=None, insert=None, drop=()):
    """The phonemiser's output for the old transcript with word i replaced by swap[i], insert[i] (a list of words) put in front
    of word i (i = number of words: behind the last) and the words of `drop` left out: (new_phns, new_word2phns, old_str,
    new_str)."""
    swap, insert = swap or {}, insert or {}
    words = old_words(case)
    new = []
    for i, (w, phs) in enumerate(words + [(None, None)]):
        new += [(x, LEX[x]) for x in insert.get(i, [])]
        if w is None or i in drop:
            continue
        new.append((swap[i], LEX[swap[i]]) if i in swap else (w, phs))
    new_phns = [ph for _, phs in new for ph in phs]
    new_w2p = {f"{i}_{w}": list(phs) for i, (w, phs) in enumerate(new)}
    return new_phns, new_w2p, " ".join(w.lower() for w, _ in words), " ".join(w.lower() for w, _ in new)


def request(fx, waves, index, max_spans=1, wav=None, **edits):
    """MultiSpanEditRequest for recorded utterance `index` rewritten by rewrite(**edits); wav: the recorded waveform by default."""
    from a3t_amd.sedit import MultiSpanEditRequest
    case = fx["cases"][index]
    new_phns, new_w2p, old_str, new_str = rewrite(case, **edits)
    wav = waves[case["wav"] + ".in"] if wav is None else wav
    return MultiSpanEditRequest(np.asarray(wav, dtype=np.float32), case["times2"], case["word2phns"], new_phns, new_w2p, old_str,
                                new_str, max_spans=max_spans, **OPTS)


def args(r):
    return (r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str)


def noise_wav(fx, waves, index, seed):
    """A waveform with a spectrum, of the recorded one's length (the recorded ones are ramps)."""
    n = waves[fx["cases"][index]["wav"] + ".in"].shape[0]
    return (0.1 * np.random.RandomState(seed).standard_normal(n)).astype(np.float32)
