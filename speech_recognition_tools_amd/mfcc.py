"""MFCC on the MI355X: the reference's baseline feature src/featgen/computeMfccFeatures.py
(extractMelEnergyFeats :58-135, driven by recipes/timit/local_pyspeech/make_mfcc_feats.sh).

Per frame (getFrames, features.py:118-154, np.hamming window, signal / 2**15):
dct(log10(|fft(frame, nfft/2 + 1)| @ createFbank(nfilters, nfft, srate).T))[:13], then spliceFeats(context).
The FFT length nfft/2 + 1 (513 at the defaults) is arbitrary, so the transform is a dense DFT on the fp64
MFMA against a twiddle matrix resident in HBM (mfcc_kernel, fdlp_mfcc.hip).
"""
import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import FdlpBatchC, FdlpMfccConfigC, check, lib, ptr


@dataclass
class MfccConfig:
    """Parsed argv of computeMfccFeatures.py (:139-150)."""
    nfilters: int = 30
    fduration: float = 0.02
    frate: int = 100
    nfft: int = 1024
    context: Optional[int] = None
    srate: int = 16000

    def to_c(self, max_frames: int) -> FdlpMfccConfigC:
        c = FdlpMfccConfigC()
        c.nfilters, c.nfft, c.frate, c.srate = int(self.nfilters), int(self.nfft), int(self.frate), int(self.srate)
        c.fduration = float(self.fduration)
        c.context = int(self.context) if self.context else 0                    # `if args.context:` (:130)
        c.max_frames = int(max_frames)
        return c


class MfccPlan:
    def __init__(self, cfg: MfccConfig, device: int = 0, max_frames: int = 65536):
        self.cfg = cfg
        self.device = device
        self.max_frames = int(max_frames)
        c = cfg.to_c(max_frames)
        h = ctypes.c_void_p()
        check(lib.fdlp_mfcc_plan_create(ctypes.byref(c), int(device), ctypes.byref(h)))
        self._h = h
        F, W = _lib.c_i32(), _lib.c_i32()
        check(lib.fdlp_mfcc_geometry(self._h, 1, ctypes.byref(F), ctypes.byref(W)))
        self.width = W.value

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            lib.fdlp_mfcc_plan_destroy(h)
            self._h = None

    def __del__(self):
        self.close()

    def frames(self, T: int) -> int:
        F = _lib.c_i32()
        check(lib.fdlp_mfcc_geometry(self._h, int(T), ctypes.byref(F), None))
        return F.value

    def tables(self):
        """Host copies of the plan's tables: dict with n, nb, K, Kpad, nbpad, ncep, nfilters, tile and the
        arrays fold [nfilters, nb], tw [Kpad, 2 nbpad], dct [nfilters, ncep] (works without a device)."""
        dims = np.zeros(8, dtype=np.int32)
        check(lib.fdlp_mfcc_plan_tables(self._h, ptr(dims, ctypes.c_int32), None, None, None))
        n, nb, K, Kpad, nbpad, ncep, nf, tile = (int(v) for v in dims)
        fold = np.zeros((nf, nb))
        tw = np.zeros((Kpad, 2 * nbpad))
        dct = np.zeros((nf, ncep))
        check(lib.fdlp_mfcc_plan_tables(self._h, ptr(dims, ctypes.c_int32), ptr(fold, ctypes.c_double),
                                        ptr(tw, ctypes.c_double), ptr(dct, ctypes.c_double)))
        return dict(n=n, nb=nb, K=K, Kpad=Kpad, nbpad=nbpad, ncep=ncep, nfilters=nf, tile=tile, fold=fold, tw=tw,
                    dct=dct)

    def compute(self, pcm: torch.Tensor, lengths: Sequence[int], offsets: Optional[Sequence[int]] = None,
                noise: Optional[torch.Tensor] = None, noise_off=None, noise_alpha=None,
                ark_decimals: int = 3, want_f64: bool = False, stream=None, preprocess=None):
        """(feats float32 [sum F, width], row offsets [n+1], feats_f64 or None) of a batch on the device.
        pcm holds the WAVs' own sample values (int16, or float64 e.g. from augment.reverb); the 2**-15
        scaling of the reference happens in the kernel.  preprocess="diff" is passed on and refused by
        fdlp_mfcc_compute (computeMfccFeatures.py has no diff option), like the sibling plans' argument."""
        if not pcm.is_cuda:
            raise ValueError("pcm must be a device tensor")
        if pcm.dtype not in (torch.int16, torch.float64):
            raise TypeError("pcm must be int16 or float64")
        kind = _lib.FDLP_PCM_I16 if pcm.dtype == torch.int16 else _lib.FDLP_PCM_F64
        pcm = pcm.contiguous()
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64))
        n = lens.size
        if offsets is None:
            offs = np.zeros(n, dtype=np.int64)
            if n:
                offs[1:] = np.cumsum(lens)[:-1]
        else:
            offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
        if n and (int((offs + lens).max()) > pcm.numel() or int(offs.min()) < 0):
            raise ValueError("utterance extends past the PCM buffer")
        Fs = np.array([self.frames(int(T)) for T in lens], dtype=np.int64)
        rows = np.zeros(n + 1, dtype=np.int64)
        rows[1:] = np.cumsum(Fs)
        total = int(rows[-1])
        out = torch.empty((total, self.width), dtype=torch.float32, device=pcm.device)
        out64 = torch.empty((total, self.width), dtype=torch.float64, device=pcm.device) if want_f64 else None
        b = FdlpBatchC()
        b.n_utt, b.pcm_kind, b.pcm_dev = n, kind, pcm.data_ptr()
        b.pcm_off, b.utt_len = ptr(offs, ctypes.c_int64), ptr(lens, ctypes.c_int64)
        if noise is not None:
            if noise.dtype != torch.int16 or not noise.is_cuda:
                raise TypeError("noise must be an int16 device tensor")
            no = np.ascontiguousarray(np.asarray(noise_off, dtype=np.int64))
            na = np.ascontiguousarray(np.asarray(noise_alpha, dtype=np.float64))
            if no.size != n or na.size != n:
                raise ValueError("one noise offset and alpha per utterance")
            if n and (int(no.min()) < 0 or int((no + lens).max()) > noise.numel()):
                raise ValueError("noise segment extends past the noise buffer")
            b.noise_dev, b.noise_off, b.noise_alpha = noise.data_ptr(), ptr(no, ctypes.c_int64), ptr(na, ctypes.c_double)
        rows_c = np.ascontiguousarray(rows[:-1])
        b.out_dev, b.out_row = out.data_ptr(), ptr(rows_c, ctypes.c_int64)
        b.out_f64_dev = out64.data_ptr() if out64 is not None else None
        b.ark_decimals = int(ark_decimals)
        if preprocess not in (None, "diff"):
            raise ValueError("preprocess must be None or 'diff'")
        b.preprocess = _lib.FDLP_PRE_DIFF if preprocess == "diff" else _lib.FDLP_PRE_NONE
        s = stream if stream is not None else torch.cuda.current_stream(pcm.device)
        check(lib.fdlp_mfcc_compute(self._h, ctypes.byref(b), ctypes.c_void_p(s.cuda_stream)))
        return out, rows, out64
