"""CPU ORACLE for the MFCC baseline feature -- TEST INFRASTRUCTURE ONLY (the checker, never the product; only
tests/ may import it).  Restatement of the reference's src/featgen/computeMfccFeatures.py (:122-131):

* frames: features.py getFrames (:118-154) on signal / 2**15, np.hamming(int(srate*fduration)), hop int(srate/frate)
* mag:    np.abs(scipy.fftpack.fft(frames, int(nfft/2 + 1), axis=1))   (a DFT of length n = nfft/2 + 1, not nfft)
* mel:    np.log10(np.matmul(mag, createFbank(nfilters, nfft, srate).T))
* mfcc:   scipy.fftpack.dct(mel, axis=1)[:, 0:13]                     (type 2, unnormalised)
* spliceFeats(mfcc, context) when context is non-zero                   (features.py:157-169)

mfcc() is that chain in float64 with scipy, as the reference runs it.  mfcc_longdouble() is the same chain in
np.longdouble from explicit tables -- cos/sin of 2 pi ((i k) mod n) / n, the filterbank with its mirrored bins
folded onto bins 0 .. n/2, the DCT-II matrix -- and returns the intermediates that cep_bound() turns into an
a-priori bound on the float64 evaluation's error.

Pinned by tests/golden/mfcc_*.npz, produced by tests/golden/make_golden_mfcc.py from the real reference.
"""
import numpy as np
import scipy.fftpack as _fp

from .mel_oracle import get_frames

U = 2.0 ** -53
NCEP = 13


def create_fbank(nfilters, nfft, srate):
    """features.py createFbank (:172-190) restated."""
    mel_max = 2595 * np.log10(1 + srate / 1400)
    fw = np.linspace(0, mel_max, nfilters + 2)
    fb = np.zeros((nfilters, int(np.floor(nfft / 2 + 1))))
    edge = np.floor((nfft + 1) * (700 * (10 ** (fw / 2595) - 1)) / srate)
    for m in range(1, nfilters + 1):
        l, c, r = int(edge[m - 1]), int(edge[m]), int(edge[m + 1])
        for k in range(l, c):
            fb[m - 1, k] = (k - edge[m - 1]) / (edge[m] - edge[m - 1])
        for k in range(c, r):
            fb[m - 1, k] = (edge[m + 1] - k) / (edge[m + 1] - edge[m])
    return fb


def splice(feats, C):
    """features.py spliceFeats (:157-169): rows F-C .. F-1 stay zero."""
    F, D = feats.shape
    out = np.zeros((F, D * (2 * C + 1)), dtype=feats.dtype)
    pad = np.concatenate([np.zeros((C, D), dtype=feats.dtype), feats, np.zeros((C, D), dtype=feats.dtype)])
    for i in range(0, F - C):
        out[i] = pad[i:i + 2 * C + 1].reshape(-1)
    return out


def mfcc(x, nfilters=30, fduration=0.02, frate=100, nfft=1024, context=None, srate=16000):
    """computeMfccFeatures.py:122-131 in float64; x is the signal entering getFrames (samples / 2**15)."""
    fr = get_frames(x, srate, frate, fduration)
    mag = np.abs(_fp.fft(fr, int(nfft / 2 + 1), axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        mel = np.log10(np.matmul(mag, np.transpose(create_fbank(nfilters, nfft, srate))))
        c = _fp.dct(mel, axis=1)[:, 0:NCEP]
    return splice(c, context) if context else c


def folded_fbank(fb):
    """fold[m,k] = fb[m,k] + fb[m,n-k] on bins 0 .. n/2 (|X[n-k]| = |X[k]| of a real frame; bin 0 and the
    Nyquist bin of an even n have no mirror), in longdouble: the sum of two doubles is exact there."""
    n = fb.shape[1]
    nb = n // 2 + 1
    fold = fb[:, :nb].astype(np.longdouble)
    for k in range(1, nb):
        if n - k != k:
            fold[:, k] += fb[:, n - k]
    return fold


def mfcc_longdouble(x, nfilters=30, fduration=0.02, frate=100, nfft=1024, context=None, srate=16000):
    """The chain in np.longdouble from the float64 frames a = x[..] * hamming (the one rounding both the reference
    and the device make before the transform).  Returns a dict: feats [F, width] (spliced when context), cep
    [F, ncep], and what cep_bound() needs -- K, abs_sum [F] = sum_i |a_i|, mag [F, nb], fold [nfilters, nb],
    w [nfilters] (non-zero bins of each filter over all n bins), lin [F, nfilters], mel, D [nfilters, ncep]."""
    ld = np.longdouble
    assert np.finfo(ld).eps < 1e-18, "np.longdouble is no wider than float64 here"
    n = int(nfft / 2 + 1)
    nb = n // 2 + 1
    fr = get_frames(x, srate, frate, fduration)
    K = min(fr.shape[1], n)                                      # fft(x, n) truncates a longer frame, pads a shorter
    a = fr[:, :K].astype(ld)
    pi = 4 * np.arctan(ld(1))
    r = (np.arange(K, dtype=np.int64)[:, None] * np.arange(nb, dtype=np.int64)[None, :]) % n
    ang = 2 * pi * r.astype(ld) / ld(n)
    mag = np.hypot(a @ np.cos(ang), a @ np.sin(ang))
    fb = create_fbank(nfilters, nfft, srate)
    fold = folded_fbank(fb)
    lin = mag @ fold.T
    with np.errstate(divide="ignore", invalid="ignore"):
        mel = np.log10(lin)
        ncep = min(NCEP, nfilters)
        m, q = np.arange(nfilters, dtype=np.int64)[:, None], np.arange(ncep, dtype=np.int64)[None, :]
        D = 2 * np.cos(pi * ((q * (2 * m + 1)) % (4 * nfilters)).astype(ld) / ld(2 * nfilters))
        cep = mel @ D
    return dict(feats=splice(cep, context) if context else cep, cep=cep, K=K, abs_sum=np.abs(a).sum(axis=1),
                mag=mag, fold=fold, w=(fb != 0).sum(axis=1), lin=lin, mel=mel, D=D, context=context)


def cep_bound(r):
    """A-priori bound on |float64 evaluation - exact| of the chain, from mfcc_longdouble()'s intermediates
    (U = 2^-53, frames a of K samples, w_m non-zero bins of filter m):

        e_mag[k] = sqrt(2) (K + 2) U sum_i |a_i|  +  4 U mag[k]       K-term dot products in any order, hypot
        e_lin[m] = sum_k fold[m,k] e_mag[k]       +  (w_m + 2) U lin[m]                  folded filterbank
        e_mel[m] = e_lin[m] / (lin[m] ln 10)      +  4 U (|mel[m]| + 1)                  log10 within a few ulp
        e_cep[q] = sum_m |D[m,q]| e_mel[m]        +  (nfilters + 2) U sum_m |mel[m] D[m,q]|          DCT-II

    Returns (e_feats [F, width], e_lin [F, nfilters]) in float64; a spliced row takes the bounds of the frames
    it copies, and the bound of a zero element is zero."""
    f = np.float64
    mag, fold, lin, mel, D = (r[k].astype(f) for k in ("mag", "fold", "lin", "mel", "D"))
    nfilters = fold.shape[0]
    e_mag = np.sqrt(2.0) * (r["K"] + 2) * U * r["abs_sum"].astype(f)[:, None] + 4 * U * mag
    e_lin = e_mag @ fold.T + (r["w"].astype(f) + 2)[None, :] * U * lin
    with np.errstate(divide="ignore", invalid="ignore"):
        e_mel = e_lin / (lin * np.log(10.0)) + 4 * U * (np.abs(mel) + 1)
        e_cep = e_mel @ np.abs(D) + (nfilters + 2) * U * (np.abs(mel) @ np.abs(D))
    return (splice(e_cep, r["context"]) if r["context"] else e_cep), e_lin
