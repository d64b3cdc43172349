"""Golden fixtures of the MFCC feature (tests/test_mfcc.py), produced by the REAL reference
src/featgen/computeMfccFeatures.py (extractMelEnergyFeats, with getKaldiArk captured: copy-feats is absent):

  mfcc_default       defaults; 4000, 2345, 700 and 5 samples (the last shorter than the reflect padding)
  mfcc_context       --context 3; the second utterance has F = 3 <= context (every row zero)
  mfcc_trunc         --nfft 512 --fduration 0.025: frames of L = 400 truncated to the DFT length n = 257
  mfcc_even_n        --nfft 254 --nfilters 8 --context 1: even DFT length n = 128, ncep = 8
  mfcc_noise_reverb  --add_noise babble,10 (np.random.seed(7)) --add_reverb small_room, short synthetic RIR;
                     the noise exceeds |181|, so int16-wrapped and float64 energies differ
  cli_options_mfcc.json   the reference's argparse table (:139-150), read from its source with ast
  mfcc_shape_<row>   the SHAPE_ROWS marked as fixtures (tests/test_mfcc_shapes.py): the tile shapes of mfcc_kernel
                     that the sets above never reach, each on shape_row_signals(); --shape-edges-only makes these
  mfcc_shape_ctx7    --nfft 2048 --context 7: F = 8 (one non-zero row), F = 5 <= context, F = 20

Run next to make_golden.py (whose signal helpers it imports):  python tests/golden/make_golden_mfcc.py
"""
import argparse
import json
import os
import sys
import tempfile
from collections import OrderedDict

import numpy as np
from scipy.io import wavfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, save, speech_like, synthetic_rir, white  # noqa: E402

MFCC_DEFAULT = dict(nfilters=30, fduration=0.02, frate=100, nfft=1024, context=None, add_noise="none",
                    add_reverb=None)


# One row per tile shape mfcc_kernel can take (tests/test_mfcc_shapes.py checks that against the plan):
# (id, options over MFCC_DEFAULT, frames per workgroup the plan picks, whether the reference's output is a fixture)
SHAPE_ROWS = [
    ("n1212", dict(nfft=1212), 32, False),                                # the largest two-row-tile shape at K = 320
    ("n1214", dict(nfft=1214), 16, False),                                # the first one-row-tile shape; 20 col tiles
    ("n1278", dict(nfft=1278), 16, False),                                # 21 column tiles: a second pass, n even
    ("n1280", dict(nfft=1280), 16, True),                                 # .. n odd
    ("n1282", dict(nfft=1282), 16, False),                                # .. n even
    ("n2048", dict(nfft=2048), 16, True),                                 # 33 column tiles, two passes
    ("n3000", dict(nfft=3000), 16, True),                                 # 47 column tiles, three passes
    ("k800", dict(nfft=1600, fduration=0.05, nfilters=64), 16, True),     # K = 800, 13 of 64 cepstra
    ("tiny", dict(nfft=32, fduration=0.002, nfilters=5), 32, True),       # K = 17, one column tile, L < hop
    ("widemel", dict(nfft=1024, fduration=0.002, nfilters=40), 32, False),  # nfilters > K
    ("oddL", dict(nfft=1024, fduration=0.0200625), 32, True),             # L = 321
    ("n636", dict(nfft=636), 32, False),                                  # n = 319 = L - 1: truncated by one sample
    ("n638", dict(nfft=638), 32, False),                                  # n = 320 = L
    ("n640", dict(nfft=640), 32, False),                                  # n = 321 = L + 1: padded by one
    ("hop533", dict(frate=30), 32, True),                                 # hop > L
    ("hop128", dict(frate=125), 32, False),
    ("empty", dict(nfft=64, nfilters=40), 32, True),                      # empty filters: non-finite rows
]
SHAPE_CTX = dict(nfft=2048, context=7)
ONE_FRAME = 5                                                             # samples: shorter than the reflect padding
# Reflect padding makes a T-sample utterance periodic with period 2 (T - 1).  At n = L = 320 a period of 8 divides
# the DFT length: the Hamming window's spectrum is then sampled at its near-zeros, the mel energies between the
# eight lines are 1e-7 of the frame's, and the error bound of their logarithms passes 1e-7 (5.2e-7; the test's
# cap).  That row's one-frame utterance has 7 samples (period 12) instead.
ONE_FRAME_OF = {"n638": 7}


def shape_row_opts(over):
    return dict(MFCC_DEFAULT, **over)


def n_frames(T, opts, srate=16000):
    """features.py getFrames (:118-154): the number of frames of T samples."""
    L, hop = int(srate * opts["fduration"]), int(srate / opts["frate"])
    lim = T - 1 if L % 2 == 0 else T
    return 0 if lim <= 0 else (lim - 1) // hop + 1


def samples_for(F, opts, srate=16000):
    """A length of F frames, away from both neighbours."""
    hop = int(srate / opts["frate"])
    T = hop * (F - 1) + 2 + min(50, hop // 2)
    assert n_frames(T, opts) == F
    return T


def shape_row_signals(index):
    """The four utterances of SHAPE_ROWS[index], of 1, M - 1, M + 1 and 2 frames with M the workgroup's frames:
    the first two fill one workgroup, the last workgroup has three live rows."""
    rid, over, M, _ = SHAPE_ROWS[index]
    opts, seed = shape_row_opts(over), 500 + 10 * index
    T1 = ONE_FRAME_OF.get(rid, ONE_FRAME)
    assert n_frames(T1, opts) == 1
    sig = OrderedDict()
    sig["s1"] = speech_like(T1, seed)
    sig["sA"] = speech_like(samples_for(M - 1, opts), seed + 1)
    sig["sB"] = white(samples_for(M + 1, opts), seed + 2)
    sig["s2"] = speech_like(samples_for(2, opts), seed + 3)
    return sig


def shape_ctx_signals():
    opts = shape_row_opts(SHAPE_CTX)
    sig = OrderedDict()
    sig["x8"] = speech_like(samples_for(8, opts), 701)      # F = context + 1: one non-zero row
    sig["x5"] = white(samples_for(5, opts), 702)            # F <= context: every row zero
    sig["x20"] = speech_like(samples_for(20, opts), 703)
    return sig


def shape_edge_fixtures():
    for i, (rid, over, _, fixture) in enumerate(SHAPE_ROWS):
        if fixture:
            sig, opts = shape_row_signals(i), shape_row_opts(over)
            save("mfcc_shape_" + rid, sig, opts, 0, run_reference_mfcc(sig, opts))
    sig, opts = shape_ctx_signals(), shape_row_opts(SHAPE_CTX)
    save("mfcc_shape_ctx7", sig, opts, 0, run_reference_mfcc(sig, opts))


def run_reference_mfcc(signals, opts, noise_seed=None, noise=None, noise_name=None, rir=None):
    sys.path.insert(0, os.path.join(REF, "src/featgen"))
    import computeMfccFeatures as cm  # noqa: E402
    captured = {}
    cm.getKaldiArk = lambda feat_dict, outfile, kaldi_cmd='copy-feats': captured.update(
        {k: np.array(v) for k, v in feat_dict.items()})
    with tempfile.TemporaryDirectory() as td:
        scp = os.path.join(td, "wav.scp")
        with open(scp, "w") as f:
            for utt, x in signals.items():
                p = os.path.join(td, utt + ".wav")
                wavfile.write(p, 16000, x)
                f.write("%s %s\n" % (utt, p))
        if noise is not None:
            os.makedirs(os.path.join(td, "noises"), exist_ok=True)
            wavfile.write(os.path.join(td, "noises", noise_name + ".wav"), 16000, noise)
        if rir is not None:
            os.makedirs(os.path.join(td, "RIR"), exist_ok=True)
            wavfile.write(os.path.join(td, "RIR", "RIR_SmallRoom1_near_AnglA.wav"), 16000, rir)
        cwd = os.getcwd()
        os.chdir(td)
        try:
            ns = argparse.Namespace(scp=scp, outfile=os.path.join(td, "out"), nfilters=opts["nfilters"],
                                    fduration=opts["fduration"], frate=opts["frate"], context=opts["context"],
                                    nfft=opts["nfft"], add_reverb=opts["add_reverb"], add_noise=opts["add_noise"],
                                    kaldi_cmd=None)
            if noise_seed is not None:
                np.random.seed(noise_seed)
            cm.extractMelEnergyFeats(ns)
        finally:
            os.chdir(cwd)
    return captured


def cli_options_fixture():
    import ast
    src = open(os.path.join(REF, "src/featgen/computeMfccFeatures.py")).read()
    opts = []
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            kw = {}
            for k in node.keywords:
                if k.arg in ("default", "action"):
                    kw[k.arg] = ast.literal_eval(k.value)
                elif k.arg == "type":
                    kw["type"] = k.value.id
            opts.append(dict(name=ast.literal_eval(node.args[0]), **kw))
    with open(os.path.join(HERE, "cli_options_mfcc.json"), "w") as f:
        json.dump(opts, f, indent=1)
    print("wrote cli_options_mfcc.json", len(opts))


def main():
    if "--shape-edges-only" in sys.argv:
        shape_edge_fixtures()
        return
    sig = OrderedDict()
    sig["c1"] = speech_like(4000, 181)
    sig["c2"] = speech_like(2345, 182)
    sig["cshort"] = white(700, 183)
    sig["ctiny"] = speech_like(5, 184)
    save("mfcc_default", sig, MFCC_DEFAULT, 0, run_reference_mfcc(sig, MFCC_DEFAULT))

    sig = OrderedDict()
    sig["x1"] = speech_like(2345, 185)
    sig["x2"] = speech_like(400, 186)   # F = 3 <= context
    opts = dict(MFCC_DEFAULT, context=3)
    save("mfcc_context", sig, opts, 0, run_reference_mfcc(sig, opts))

    sig = OrderedDict()
    sig["t1"] = speech_like(3000, 187)
    sig["t2"] = white(401, 188)
    opts = dict(MFCC_DEFAULT, nfft=512, fduration=0.025)
    save("mfcc_trunc", sig, opts, 0, run_reference_mfcc(sig, opts))

    sig = OrderedDict()
    sig["e1"] = speech_like(2000, 189)
    sig["e2"] = speech_like(333, 190)
    opts = dict(MFCC_DEFAULT, nfft=254, nfilters=8, context=1)
    save("mfcc_even_n", sig, opts, 0, run_reference_mfcc(sig, opts))

    sig = OrderedDict()
    sig["n1"] = speech_like(4000, 191)
    sig["n2"] = speech_like(2345, 192)
    rir = synthetic_rir(300, 193)
    noise = white(12000, 194, scale=1000.0)
    assert np.abs(noise).max() > 181
    opts = dict(MFCC_DEFAULT, add_noise="babble,10", add_reverb="small_room")
    save("mfcc_noise_reverb", sig, opts, 0,
         run_reference_mfcc(sig, opts, noise_seed=7, noise=noise, noise_name="babble", rir=rir),
         extra=dict(noise_seed=7), more={"rir": rir, "noise_babble": noise})
    cli_options_fixture()
    shape_edge_fixtures()


if __name__ == "__main__":
    main()
