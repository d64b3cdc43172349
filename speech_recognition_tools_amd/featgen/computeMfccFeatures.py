#!/usr/bin/env python3
"""compute-mfcc-feats: argv-compatible drop-in for sadhusamik/speech_recognition_tools
src/featgen/computeMfccFeatures.py (argparse table :139-150, extractMelEnergyFeats :58-135), the MFCC
baseline feature of recipes/timit/local_pyspeech/make_mfcc_feats.sh, running on an MI355X
(speech_recognition_tools_amd.mfcc, mfcc_kernel).

Same positional arguments, options, defaults and outputs (<outfile>.ark/.scp); the ark is written natively
with the reference's '%.3f' rounding (getKaldiArk :26-32), so --kaldi_cmd is accepted and ignored.
Additions: --noise_seed (np.random seed of the noise offsets), --device, --batch_frames, --io_workers,
--ark_precision.
"""
import argparse
import os
import sys

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def get_args(argv=None):
    parser = argparse.ArgumentParser('Extract Mel Energy Features')
    parser.add_argument('scp', help='"scp" list')
    parser.add_argument('outfile', help='output file')
    parser.add_argument('--nfilters', type=int, default=30, help='number of filters (30)')
    parser.add_argument('--fduration', type=float, default=0.02, help='Window length (0.02 sec)')
    parser.add_argument('--frate', type=int, default=100, help='Frame rate (100 Hz)')
    parser.add_argument('--context', type=int, help='Frame Context')
    parser.add_argument('--nfft', type=int, default=1024, help='Number of points of computing FFT')
    parser.add_argument('--add_reverb', help='input "clean" OR "small_room" OR "large_room"')
    parser.add_argument('--add_noise', help='Specify "type of noise, snr" if not specify none', default='none')
    parser.add_argument('--kaldi_cmd', help='Kaldi command to use to get ark files')
    # MI355X additions (all optional)
    parser.add_argument('--noise_seed', type=int, default=None, help='seed of the noise offsets (np.random.seed)')
    parser.add_argument('--device', type=int, default=None, help='HIP device (default: LOCAL_RANK or 0)')
    parser.add_argument('--batch_frames', type=int, default=65536, help='frames per GPU batch')
    parser.add_argument('--io_workers', type=int, default=4, help='threads reading `<cmd> |` scp entries ahead (plain files are read inline)')
    parser.add_argument('--ark_precision', type=int, default=3, help="decimals of the text ark ('%%.3f')")
    return parser.parse_args(argv)


MFCC_ROOMS = ('small_room', 'large_room')  # :81-88; this script has no medium_room


def extractMelEnergyFeats(args, srate=16000, window=np.hamming, return_feats=False):
    """computeMfccFeatures.py:58-135 on the device."""
    if window is not np.hamming:
        raise ValueError("only the reference's np.hamming analysis window is supported")
    import collections

    import torch
    from speech_recognition_tools_amd import NpRandom
    from speech_recognition_tools_amd.augment import load_rir, noise_params_f64, reverb
    from speech_recognition_tools_amd.featgen.features import load_noise
    from speech_recognition_tools_amd.io_pipeline import ArkStream, PrefetchReader
    from speech_recognition_tools_amd.mfcc import MfccConfig, MfccPlan

    cfg = MfccConfig(nfilters=args.nfilters, fduration=args.fduration, frate=args.frate, nfft=args.nfft,
                     context=args.context, srate=srate)
    add_noise, add_reverb = args.add_noise, args.add_reverb
    noise = None
    if add_noise != "none":                                                  # :76-78
        noise_info = add_noise.strip().split(',')
        noise = load_noise(noise_info[0])
        snr = float(noise_info[1])
    rir = None
    if add_reverb:                                                           # :80-93
        if add_reverb in MFCC_ROOMS:
            rir = load_rir(add_reverb)
        elif add_reverb == 'clean':
            print('%s: No reverberation added!' % sys.argv[0])
        else:
            raise ValueError('Invalid type of reverberation!')
        sys.stdout.flush()
    device = args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(device)
    plan = MfccPlan(cfg, device=device, max_frames=max(int(args.batch_frames), 1))
    dev = torch.device("cuda", device)
    noise_rng = NpRandom(args.noise_seed) if noise is not None else None
    noise_dev = torch.from_numpy(np.ascontiguousarray(noise)).to(dev) if noise is not None else None
    rir_dev = torch.from_numpy(np.ascontiguousarray(rir, dtype=np.float64)).to(dev) if rir is not None else None

    feats_out = collections.OrderedDict() if return_feats else None
    ark = ArkStream(args.outfile)
    pending, pending_frames = [], 0

    def flush():
        nonlocal pending, pending_frames
        if not pending:
            return
        lens = [x[1].shape[0] for x in pending]
        pcm = torch.from_numpy(np.concatenate([x[1] for x in pending])).pin_memory().to(dev, non_blocking=True)
        kw = {}
        if noise is not None and pcm.dtype == torch.int16:                   # float64 signals were mixed on the host
            kw = dict(noise=noise_dev, noise_off=[x[2] for x in pending], noise_alpha=[x[3] for x in pending])
        offs = None
        if rir_dev is not None:                                              # :118-120, after the noise
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            pcm, lens = reverb(pcm, lens, rir_dev, offsets=offs, **kw)
            kw = {}
        out, rows, _ = plan.compute(pcm, lens, offsets=offs, ark_decimals=args.ark_precision, **kw)
        host = out.cpu().numpy()
        for i, x in enumerate(pending):
            m = host[rows[i]:rows[i + 1]]
            ark.write(x[0], m)
            if feats_out is not None:
                feats_out[x[0]] = m.copy()
        pending, pending_frames = [], 0

    try:
        for uttid, sig, sr in PrefetchReader(args.scp, 'wav', workers=args.io_workers):     # :95-110
            print('%s: Computing Features for file: %s' % (sys.argv[0], uttid))
            sys.stdout.flush()
            if sig is None:
                continue
            assert sr == srate, 'Input file has different sampling rate.'    # :111
            if sig.ndim != 1:
                raise ValueError("multi-channel WAV input is not supported (the reference expects mono)")
            off, alpha = 0, 0.0
            if noise is not None:                                            # :115-116
                off, alpha = noise_params_f64(sig, noise, snr, noise_rng.rand())
                if sig.dtype != np.int16:  # the device mixes int16 signals; any other dtype is mixed here
                    sig = np.asarray(sig, dtype=np.float64) + alpha * noise[off:off + sig.shape[0]].astype(np.float64)
            if sig.dtype != np.int16:
                sig = np.ascontiguousarray(sig, dtype=np.float64)
            F = plan.frames(sig.shape[0])
            if F < 1:
                raise ValueError("utterance %s (%d samples) has no analysis frame" % (uttid, sig.shape[0]))
            if pending and (pending_frames + F > plan.max_frames or pending[0][1].dtype != sig.dtype):
                flush()
            if F > plan.max_frames:
                plan = MfccPlan(cfg, device=device, max_frames=F)
            pending.append((uttid, sig, off, alpha))
            pending_frames += F
        flush()
    except BaseException:  # a failed JOB publishes no partial ark/scp (fdlp_ark_abort)
        ark.abort()
        raise
    finally:
        ark.close()
    return feats_out


if __name__ == '__main__':
    extractMelEnergyFeats(get_args())
