"""Golden fixtures of the MFCC feature (tests/test_mfcc.py), produced by the REAL reference
src/featgen/computeMfccFeatures.py (extractMelEnergyFeats, with getKaldiArk captured: copy-feats is absent):

  mfcc_default       defaults; 4000, 2345, 700 and 5 samples (the last shorter than the reflect padding)
  mfcc_context       --context 3; the second utterance has F = 3 <= context (every row zero)
  mfcc_trunc         --nfft 512 --fduration 0.025: frames of L = 400 truncated to the DFT length n = 257
  mfcc_even_n        --nfft 254 --nfilters 8 --context 1: even DFT length n = 128, ncep = 8
  mfcc_noise_reverb  --add_noise babble,10 (np.random.seed(7)) --add_reverb small_room, short synthetic RIR;
                     the noise exceeds |181|, so int16-wrapped and float64 energies differ
  cli_options_mfcc.json   the reference's argparse table (:139-150), read from its source with ast

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


if __name__ == "__main__":
    main()
