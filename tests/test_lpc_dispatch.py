"""Every kernel the Levinson -> cepstrum -> envelope stage can dispatch to, against the CPU oracle.

launch_lpc_env (csrc/fdlp_lpc.hip) picks lpc_env_lattice_kernel<SL, CB, DM>, an external Durbin
(durbin4_kernel<38>, durbin8_kernel<17|19|21|23>) or the LDS kernel lpc_env_kernel<TS> from order, coeff_num,
fduration * frate and the plan mode, and the envelope has branches of its own (the FFT route at Me = 300,
a second Chebyshev chunk from env_nfft 320, the cosine-table modulo below env_nfft 80, the odd-Me tail, odd
H = env_nfft / 2).  DISPATCH_CASES below holds one small batch per reachable instantiation and branch:

* test_table_covers_dispatch_space (CPU): FdlpPlan.lpc_dispatch() of host-only plans over the table, for the
  'auto', 'lattice8' and 'lds' paths, reaches every SL, CB, DM, Durbin kernel and TS the launcher can pick, so
  a changed dispatch threshold fails here until the table follows it.  (One combination cannot occur and is
  asserted absent: CB != 0 needs SL 9..11, p 128..175, which lies inside durbin8_kernel's p 120..183, so
  the register cepstra never run with the in-register Durbin.)
* test_inputs_are_well_conditioned (CPU): the bar of every row is 8 x the oracle's own movement when each
  autocorrelation moves by 1e-12 r0 N(0, 1) (the bar the suite holds the device r to), maximum of 3 seeds,
  separately for the cepstra, log env[..., 1:-1] and the features; every feature bar stays below 1e-6.
* test_row_* (GPU): shapes, r within 1e-12 r0, a / gg of every item against solve_toeplitz on the device's
  own r (1e-9 / 1e-11), cep, log env and the fp64 features within the row's bars, float32 within one 0.001
  step, through 'auto', 'lds' and (where the dispatch differs) 'lattice8', the paths agreeing within the
  bar, and the Durbin kernel lpc_dispatch() names being the one kernel_times() saw launched.
* test_persistent_grid_* (GPU): more than 8 item groups per resident block of the persistent lattice kernel.
* test_rows_under_range_checks (GPU): every row once under the range-check build, zero violations.

`python tests/test_lpc_dispatch.py --record` (on the device) rewrites tests/data/lpc_dispatch_errors.jsonl,
the per-row maxima next to their bars.  MEASURED_WORST below quotes the worst error / bar ratios of that file:
0.25 on r (row 55, 247 mel bands of one to three taps), 0.00052 on gg (row 42, 'lattice8'), 0.00049 on a (row 53),
0.00012 on the features and on log env and 0.00006 on the cepstra (row 00, 'lds');
test_recorded_errors_match_docstring keeps the two equal.
"""
import functools
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
from scipy.signal import lfilter

from conftest import ROOT
from oracle import fdlp_oracle as O
from oracle import mel_oracle as MO
from oracle import modspec_oracle as MS

COCH = "cochlear,1,1,1,2.5,1"   # the structured autocorrelation runs in front of the LPC stage
MEL = "mel,1"                   # the direct autocorrelation
NF = 7                          # bands: 3 frames x 7 = 21 items at fduration 0.5, no multiple of 4, 8 or 16
SEED = 5                        # hop jitter
PERTURB = 1e-12                 # of r0: the suite's bar on the device autocorrelation
MARGIN = 8.0                    # bar = MARGIN x the oracle's movement under PERTURB
FEATURE_CAP = 1e-6              # no row's feature bar may exceed this
A_FLOOR, GG_FLOOR = 1e-9, 1e-11  # per item against solve_toeplitz (test_gpu_parity.assert_durbin4_accuracy)
ERRORS_FILE = os.path.join(ROOT, "tests", "data", "lpc_dispatch_errors.jsonl")
CHECKS_LIB = os.path.join(ROOT, "speech_recognition_tools_amd", "lib", "libfdlp_checks.so")

# Worst error / bar ratio per quantity over tests/data/lpc_dispatch_errors.jsonl (all rows, all paths), as
# (ratio, row, path): filled from the recorded file, test_recorded_errors_match_docstring compares them.
# Every path of every row is three to four orders of magnitude inside its bar (largest absolute errors:
# a 4.9e-13, gg 5.2e-15, cep 2.4e-13, log env 2.7e-12, features 2.0e-12 against feature bars of 4.3e-11 ..
# 4.8e-7; the float32 rows equal the rounded oracle's), so no margin was widened and no kernel changed.  The one
# exception is r of row 55 (247 mel bands at N = 1600, one to three taps each): 2.5e-13 r0, a quarter of the
# suite's 1e-12 bar on the device autocorrelation; its a, gg, cepstra and features are as far inside as the rest.
MEASURED_WORST = {
    "a": (0.000494, "53-mel-fd0.1-fr100-p20-M15-spectrogram", "auto"),
    "gg": (0.000521, "42-cochlear-fd1.5-fr100-p150-M300-spectrogram", "lattice8"),
    "r": (0.248, "55-mel-fd0.1-fr100-p12-M10-spectrogram", "auto"),
    "cep": (6.24e-05, "00-cochlear-fd0.5-fr100-p1-M20-spectrogram", "lds"),
    "env": (0.000117, "00-cochlear-fd0.5-fr100-p1-M20-spectrogram", "lds"),
    "feat": (0.000123, "00-cochlear-fd0.5-fr100-p1-M20-spectrogram", "lds"),
}


def _spec(fb, fd, fr, order, cn):
    return (fb, NF, fd, fr, order, cn, "spectrogram")


def _mod(fb, order, cn, c0, mode="modspec", **kw):
    return (fb, NF, 0.5, 100, order, cn, mode, dict(coeff_0=c0, no_window=True, **kw))


# (fbank, nfilters, fduration, frate, order, coeff_num, mode[, modspec options]); coeff_num is --coeff_n in
# the modspec modes.  About a third of the rows use the mel filterbank.
DISPATCH_CASES = [
    # ---- order x coeff_num at fduration 0.5, frate 100 (env_nfft 100, kk 50) ----
    _spec(COCH, 0.5, 100, 1, 20),       # SL 1, M > p + 1
    _spec(MEL, 0.5, 100, 15, 16),       # SL 1, p + 1 = 16 fills the lanes, M = p + 1
    _spec(COCH, 0.5, 100, 16, 40),      # SL 2
    _spec(COCH, 0.5, 100, 47, 100),     # SL 3
    _spec(MEL, 0.5, 100, 63, 64),       # SL 4, M = p + 1
    _spec(COCH, 0.5, 100, 64, 64),      # SL 5, M < p + 1
    _spec(COCH, 0.5, 100, 79, 113),     # SL 5, odd M
    _spec(MEL, 0.5, 100, 80, 112),      # SL 6
    _spec(COCH, 0.5, 100, 96, 100),     # SL 7
    _spec(COCH, 0.5, 100, 111, 101),    # SL 7, odd M
    _spec(MEL, 0.5, 100, 112, 100),     # SL 8, in-register Durbin just below durbin8's range
    _spec(COCH, 0.5, 100, 119, 100),    # SL 8, the last order below durbin8's range
    _spec(COCH, 0.5, 100, 120, 100),    # SL 8, durbin8<17>, CB 0 with an external Durbin
    _spec(COCH, 0.5, 100, 127, 300),    # SL 8, durbin8<17>, M > p + 1
    _spec(MEL, 0.5, 100, 128, 100),     # SL 9, CB 7, durbin4 at its first order
    _spec(MEL, 0.5, 100, 135, 450),     # SL 9, CB -1, durbin4 (lattice8: durbin8<17>)
    _spec(COCH, 0.5, 100, 143, 112),    # SL 9, CB 7 at its largest M (lattice8: durbin8<19>)
    _spec(COCH, 0.5, 100, 143, 113),    # SL 9, CB -1 at its smallest M
    _spec(MEL, 0.5, 100, 151, 100),     # SL 10, CB 7, durbin8<19> by default
    _spec(COCH, 0.5, 100, 159, 113),    # SL 10, CB -1, durbin8<21>
    _spec(COCH, 0.5, 100, 160, 100),    # SL 11, CB 7, durbin8<21>
    _spec(MEL, 0.5, 100, 160, 450),     # SL 11, CB -1
    _spec(COCH, 0.5, 100, 175, 112),    # SL 11, CB 7, durbin8<23>
    _spec(COCH, 0.5, 100, 176, 100),    # SL 12, CB 0, durbin8<23>
    _spec(MEL, 0.5, 100, 183, 113),     # SL 12, durbin8<23> at its last order
    _spec(COCH, 0.5, 100, 184, 184),    # SL 12, the in-register Durbin again
    _spec(COCH, 0.5, 100, 207, 100),    # SL 13
    _spec(MEL, 0.5, 100, 223, 101),     # SL 14
    _spec(COCH, 0.5, 100, 238, 100),    # SL 15, the largest order
    _spec(COCH, 0.5, 100, 238, 450),    # SL 15, M > p + 1
    _spec(MEL, 0.5, 100, 150, 2),       # Me 2: the envelope loop never runs, only the tail
    _spec(COCH, 0.5, 100, 150, 3),      # Me 3: one loop trip, no tail
    # ---- envelope geometries ----
    _spec(COCH, 0.5, 60, 150, 100),     # env_nfft 60: the cosine-table modulo, Me 60
    _spec(MEL, 0.5, 60, 50, 50),
    _spec(COCH, 0.5, 103, 150, 100),    # kk 52, env_nfft 102, H 51 odd, kk = H + 1
    _spec(MEL, 0.5, 103, 60, 113),      # Me 102
    _spec(COCH, 0.1, 100, 40, 15),      # N 1600, env_nfft 20, Me 15 odd
    _spec(MEL, 0.064, 125, 20, 8),      # N 1024, the plan's minimum; env_nfft 16
    _spec(COCH, 1.0, 160, 150, 100),    # env_nfft 320: the second Chebyshev chunk
    _spec(MEL, 1.0, 238, 150, 450),     # kk 238, env_nfft 476, TS 8
    _spec(COCH, 1.5, 109, 150, 100),    # env_nfft 326 = 2 mod 4, kk 164
    _spec(COCH, 1.5, 100, 150, 299),    # Me 299: just below the env_fft300 condition, odd Me
    _spec(COCH, 1.5, 100, 150, 300),    # the env_fft300 route
    _spec(MEL, 1.5, 100, 150, 301),     # Me 300 with M 301: the FFT route with one coefficient cut
    # ---- modulation spectrum (kk 1, env_nfft 2, Me 2): (order, coeff_n, coeff_0) ----
    # With --no_window: under the default hanning window the frame's temporal envelope, which the LPC models,
    # falls to zero at both frame ends, and these orders are then ill conditioned for ANY input (order 150,
    # N 8000: the features move by 2.8e-5 on the speech-like and 1.6e-6 on the white utterance under the
    # 1e-12 r0 perturbation, against the 1e-6 cap on 8 x that).  The window is applied before the DCT and does
    # not reach the LPC dispatch; the rectangular frames move by 1e-10 .. 7e-10.  The hanning window itself
    # is covered by the modspec_* golden sets (tests/test_modspec.py).
    _mod(MEL, 150, 100, 1),                     # CB 7, durbin4
    _mod(COCH, 160, 120, 5),                    # CB -1, durbin8<21>
    _mod(MEL, 120, 30, 5),                      # CB 0, durbin8<17>
    _mod(COCH, 135, 113, 2, keep_even=True),    # CB -1, durbin4, odd coeff_n
    _mod(MEL, 200, 260, 1),                     # CB 0, M > p + 1, SL 13
    _mod(COCH, 64, 130, 1),                     # CB 0, M > p + 1, SL 5
    # ---- complex modulation spectrum (cplx_lpc_out_kernel): two, three and four trips of its lane loops ----
    _mod(MEL, 65, 70, 1, mode="modspec_complex"),
    _mod(MEL, 129, 130, 5, mode="modspec_complex", absolute_value=True),
    _mod(MEL, 238, 260, 1, mode="modspec_complex"),
    # ---- more than 80 bands: the output stage's LDS loop behind the whole pipeline (tests/test_ola_stage.py
    # holds that stage alone); 247 bands is the first count whose launch needs the large-LDS attribute ----
    (MEL, 81, 0.1, 100, 20, 15, "spectrogram"),
    (COCH, 81, 0.5, 100, 30, 30, "spectrogram"),
    (MEL, 247, 0.1, 100, 12, 10, "spectrogram"),
]
ROW_IDS = ["%02d-%s-fd%g-fr%d-p%d-M%d-%s" % (i, r[0].split(",")[0], r[2], r[3], r[4], r[5], r[6])
           for i, r in enumerate(DISPATCH_CASES)]
SPEC_ROWS = [i for i, r in enumerate(DISPATCH_CASES) if r[6] == "spectrogram"]
MOD_ROWS = [i for i, r in enumerate(DISPATCH_CASES) if r[6] == "modspec"]
CPLX_ROWS = [i for i, r in enumerate(DISPATCH_CASES) if r[6] == "modspec_complex"]
LPC_PATHS = ("auto", "lattice8", "lds")


# ---- inputs (the recipes of tests/golden/make_golden.py) ------------------------------------------------
def speech_like(T, seed, rms=2000.0):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(T + 400)
    f0 = rng.uniform(400, 1500)
    rad = rng.uniform(0.90, 0.98)
    a1, a2 = -2 * rad * np.cos(2 * np.pi * f0 / 16000), rad * rad
    x = lfilter([1.0], [1.0, a1, a2], e)[400:]
    t = np.arange(T) / 16000
    env = 0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(3, 5) * t + rng.uniform(0, 6.28))
    x = x * env
    x = x / (np.sqrt(np.mean(x ** 2)) + 1e-12) * rms
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def white(T, seed, scale=3000.0):
    x = np.random.default_rng(seed).standard_normal(T) * scale
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def row_opts(row):
    return row[7] if len(row) > 7 else {}


def row_signals(row):
    """Two utterances, speech-like and white: 12000 and 5000 samples (30000 and 40000 from fduration 1.0)."""
    T1, T2 = (30000, 40000) if row[2] >= 1.0 else (12000, 5000)
    return [speech_like(T1, 11), white(T2, 12)]


def feature_config(row, nfilters=None):
    from speech_recognition_tools_amd import FeatureConfig
    fb, nf, fd, fr, order, cn, mode = row[:7]
    o = row_opts(row)
    if mode == "spectrogram":
        return FeatureConfig(fbank_type=fb, nfilters=nfilters or nf, fduration=fd, frate=fr, order=order,
                             coeff_num=cn, coeff_range="0,%d" % cn)
    return FeatureConfig(mode=mode, window="rect" if o.get("no_window") else "hanning", fbank_type=fb,
                         nfilters=nf, fduration=fd, frate=fr,
                         order=order, coeff_num=cn, coeff_0=o["coeff_0"], keep_even=bool(o.get("keep_even")),
                         absolute_value=bool(o.get("absolute_value")))


def oracle_config(row, nfilters=None):
    fb, nf, fd, fr, order, cn = row[:6]
    return O.FdlpConfig(fbank_type=fb, nfilters=nfilters or nf, fduration=fd, frate=fr, order=order, coeff_num=cn,
                        coeff_range="0,%d" % cn)


def modspec_kwargs(row):
    fb, nf, fd, fr, order, cn = row[:6]
    o = row_opts(row)
    return dict(nfilters=nf, coeff_0=o["coeff_0"], coeff_n=cn, order=order, fduration=fd, frate=fr, fbank_type=fb,
                keep_even=bool(o.get("keep_even")), absolute_value=bool(o.get("absolute_value")),
                no_window=bool(o.get("no_window")))


def host_dispatch(row, lpc):
    from speech_recognition_tools_amd import FdlpPlan
    plan = FdlpPlan(feature_config(row), device=-1, max_frames=16)
    plan.set_lpc_path(lpc)
    return plan.lpc_dispatch()


# ---- 3. the table covers the dispatch space --------------------------------------------------------------
def test_table_covers_dispatch_space():
    seen = set()     # (SL, CB, DM, Durbin kernel, SL8, M > p + 1) of the lattice kernel
    ts_lds = set()
    for row in DISPATCH_CASES:
        p, M = row[4], row[5]
        for lpc in LPC_PATHS:
            d = host_dispatch(row, lpc)
            assert d["lpc_blocks"] == 0  # host-only plan
            kind, sl8 = d["durbin"]
            if kind == "cplx":
                assert row[6] == "modspec_complex"
                continue
            if kind == "lds":
                assert lpc == "lds" and d["SL"] == 0 and d["DM"] is None
                ts_lds.add(d["TS"])
                continue
            assert lpc != "lds" and d["SL"] == (p + 1 + 15) // 16 and d["TS"] == 0
            assert (d["DM"] == "ext") == (kind in ("durbin4", "durbin8"))
            seen.add((d["SL"], d["CB"], d["DM"], kind, sl8, M > p + 1))
    assert {s[0] for s in seen} == set(range(1, 16))
    for sl in (9, 10, 11):
        for cb in (7, -1):
            assert any(s[0] == sl and s[1] == cb for s in seen), (sl, cb)
    assert {s[1] for s in seen} == {7, -1, 0}
    assert any(s[1] == 0 and s[5] for s in seen) and any(s[1] == 0 and not s[5] for s in seen)
    assert any(s[3] == "durbin4" for s in seen)
    assert {s[4] for s in seen if s[3] == "durbin8"} == {17, 19, 21, 23}
    # durbin8 at each SL8 is also a default choice, not only the 'lattice8' cross-check
    auto = {host_dispatch(row, "auto")["durbin"] for row in DISPATCH_CASES}
    assert {("durbin8", k) for k in (17, 19, 21, 23)} <= auto and ("durbin4", 0) in auto and ("inreg", 0) in auto
    # both Durbin modes with the LDS cepstrum; the register cepstra (SL 9..11, p 128..175) lie inside
    # durbin8_kernel's range (p 120..183), so they only ever follow an external Durbin
    assert any(s[1] == 0 and s[2] == "contig" for s in seen) and any(s[1] == 0 and s[2] == "ext" for s in seen)
    assert any(s[1] != 0 and s[2] == "ext" for s in seen)
    assert not any(s[1] != 0 and s[2] == "contig" for s in seen)
    assert len(ts_lds) >= 4, ts_lds
    # every threshold of the default dispatch is bracketed by two rows one step apart, so moving one by a
    # single step already changes what some row of the table dispatches to
    by_pm = {(row[4], row[5]): host_dispatch(row, "auto") for row in DISPATCH_CASES if row[6] == "spectrogram"
             and row[2] == 0.5 and row[3] == 100}
    assert by_pm[(143, 112)]["CB"] == 7 and by_pm[(143, 113)]["CB"] == -1      # register / window cepstrum
    assert by_pm[(119, 100)]["durbin"] == ("inreg", 0) and by_pm[(120, 100)]["durbin"] == ("durbin8", 17)
    assert by_pm[(127, 300)]["durbin"] == ("durbin8", 17) and by_pm[(128, 100)]["durbin"] == ("durbin4", 0)
    assert by_pm[(150, 2)]["durbin"] == ("durbin4", 0) and by_pm[(151, 100)]["durbin"] == ("durbin8", 19)
    assert by_pm[(183, 113)]["durbin"] == ("durbin8", 23) and by_pm[(184, 184)]["durbin"] == ("inreg", 0)
    assert by_pm[(175, 112)]["CB"] == 7 and by_pm[(176, 100)]["CB"] == 0        # SL 11 / 12
    assert by_pm[(127, 300)]["CB"] == 0 and by_pm[(128, 100)]["CB"] == 7        # SL 8 / 9
    # envelope geometries of the spectrogram rows
    geo = [O.geometry(oracle_config(DISPATCH_CASES[i])) for i in SPEC_ROWS]
    me = [min(DISPATCH_CASES[i][5], g.env_nfft) for i, g in zip(SPEC_ROWS, geo)]
    assert any(m % 2 for m in me) and any(m % 2 == 0 for m in me)
    assert any(g.env_nfft < 80 for g in geo) and any(g.env_nfft >= 320 for g in geo)
    assert any(g.env_nfft % 4 == 2 for g in geo)
    assert any(g.env_nfft == 300 and m == 300 and g.kk == 150 for g, m in zip(geo, me))  # the FFT route
    assert {299, 300} <= set(me)


def test_host_plan_records_lpc_path():
    """fdlp_set_lpc_path on a host-only plan records the path for lpc_dispatch; the recipes' dispatch."""
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig
    plan = FdlpPlan(FeatureConfig.wsj(), device=-1)
    assert plan.lpc_dispatch() == dict(SL=10, CB=7, DM="ext", durbin=("durbin4", 0), TS=0, lpc_blocks=0)
    plan.set_lpc_path("lattice8")
    assert plan.lpc_dispatch()["durbin"] == ("durbin8", 19)
    plan.set_lpc_path("lds")
    assert plan.lpc_dispatch() == dict(SL=0, CB=0, DM=None, durbin=("lds", 0), TS=5, lpc_blocks=0)
    plan = FdlpPlan(FeatureConfig.reverb(), device=-1)
    assert (plan.lpc_dispatch()["SL"], plan.lpc_dispatch()["CB"]) == (10, -1)


# ---- the oracle's chain from the autocorrelation on, and its movement under a perturbed r ---------------
def lpc_chain(r, p):
    """a [n, p+1], gg [n] of autocorrelation rows (real or complex), each item as features.py:226-228."""
    a = np.empty((r.shape[0], p + 1), dtype=r.dtype)
    gg = np.empty(r.shape[0], dtype=r.dtype)
    for t in range(r.shape[0]):
        a[t], gg[t] = O.lpc_from_autocorr(r[t], p)
    return a, gg


def complex_cepstrum_batch(a, gg, M):
    """modspec_oracle.complex_cepstrum over a batch (the same products in the same order per item)."""
    n_it, p1 = a.shape
    x = np.zeros((n_it, max(p1, M + 1)), dtype=np.complex128)
    x[:, 1:p1] = -a[:, 1:]
    c = np.zeros((n_it, M), dtype=np.complex128)
    c[:, 0] = np.log(np.sqrt(gg))
    c[:, 1] = x[:, 1]
    for n in range(2, M):
        aa = np.arange(1, n) / n
        c[:, n] = np.sum(aa[None, :] * x[:, n - 1:0:-1] * c[:, 1:n], axis=1) + x[:, n]
    return c


def perturbed(r, seed):
    rng = np.random.default_rng(1000 + seed)
    s = PERTURB * np.abs(r[:, :1])
    if np.iscomplexobj(r):
        return r + s * (rng.standard_normal(r.shape) + 1j * rng.standard_normal(r.shape))
    return r + s * rng.standard_normal(r.shape)


def log_env(env):
    return np.log(env[..., 1:-1])


class Reference:
    """Oracle outputs of one row and the bars derived from the oracle's own movement."""


@functools.lru_cache(maxsize=None)
def spectro_reference(idx):
    row = DISPATCH_CASES[idx]
    orc = O.FdlpOracle(oracle_config(row))
    p, M, B = row[4], row[5], row[1]
    sigs = row_signals(row)
    rng, rng2 = random.Random(SEED), random.Random(SEED)
    ref = Reference()
    ref.feats, keeps, jits = [], [], []
    for x in sigs:
        keep = O.Intermediates()
        ref.feats.append(orc.utterance(x, rng, keep))
        keeps.append(keep)
        jits.append([rng2.randrange(2) for _ in range(keep.r.shape[0] - 1)])
    ref.r = np.concatenate([k.r for k in keeps]).reshape(-1, p + 2)
    ref.cep = np.concatenate([k.cep for k in keeps]).reshape(-1, M)
    ref.env = np.concatenate([k.env for k in keeps]).reshape(ref.r.shape[0], -1)
    ref.nframes = ref.r.shape[0] // B
    assert (ref.r[:, 0] > 0).all()

    def chain(r):
        a, gg = lpc_chain(r, p)
        cep = O.cepstrum_batch(a, gg, M)
        env = O.envelope_batch(cep * orc.w[None, :], orc.g)
        feats, f0 = [], 0
        for x, k, jit in zip(sigs, keeps, jits):
            F = k.r.shape[0]
            feats.append(O.ola_features(env[f0 * B:(f0 + F) * B].reshape(F, B, -1), x.size, jit, orc.cfg, orc.g))
            f0 += F
        return cep, env, feats

    cep0, env0, feats0 = chain(ref.r)  # the restated chain is the oracle's, bit for bit
    assert np.array_equal(cep0, ref.cep) and np.array_equal(env0, ref.env)
    assert all(np.array_equal(a, b) for a, b in zip(feats0, ref.feats))
    mv = np.zeros(3)
    for seed in range(3):
        cep, env, feats = chain(perturbed(ref.r, seed))
        mv = np.maximum(mv, [np.abs(cep - ref.cep).max(), np.abs(log_env(env) - log_env(ref.env)).max(),
                             max(np.abs(a - b).max() for a, b in zip(feats, ref.feats))])
    ref.bar_cep, ref.bar_env, ref.bar_feat = (MARGIN * mv).tolist()
    return ref


def modspec_select(mod, coeff_0, coeff_n, keep_even, absolute_value, cplx):
    """[items, width]: the slice of computeModulationSpectrum.py:184-197 (modspec_oracle)."""
    sel = mod[:, coeff_0 - 1:coeff_n]
    if cplx:
        sel = np.abs(sel) if absolute_value else np.concatenate([sel.real, sel.imag], axis=1)
    elif absolute_value:
        sel = np.abs(sel)
    if keep_even:
        sel = sel[:, 1::2] if coeff_0 % 2 == 0 else sel[:, 0::2]
    return sel


@functools.lru_cache(maxsize=None)
def modspec_reference(idx):
    import scipy.fftpack as fp
    row = DISPATCH_CASES[idx]
    fb_t, B, fd, fr, p, M, mode = row[:7]
    kw = modspec_kwargs(row)
    cplx = mode == "modspec_complex"
    N = int(16000 * fd)
    sigs = row_signals(row)
    ref = Reference()
    ref.feats, rs = [], []
    for x in sigs:
        xf = x.astype(np.float64)
        ref.feats.append((MS.modspec_complex_features if cplx else MS.modspec_features)(xf, **kw))
        fr_ = MO.get_frames(xf, 16000, fr, fd, (lambda n: np.ones(n)) if kw["no_window"] else np.hanning)
        if cplx:  # modspec_oracle.modspec_complex_features, the autocorrelation of every (frame, band)
            fb = MO.mel_fbank(B, N, 16000, fb_t)
            X = fp.ifft(fr_)[:, :int(fd * 16000 / 2)]
            S = np.fft.fft(fb[None, :, :-1] * X[:, None, :], axis=-1)
            rs.append(np.fft.ifft(S * np.conj(S), axis=-1)[..., :p + 2].reshape(-1, p + 2))
        else:
            fb = MO.mel_fbank(B, int(2 * fd * 16000), 16000, fb_t)
            D = fp.dct(fr_) / np.sqrt(2 * N)
            rs.append(O.autocorr_fft((fb[None, :, :-1] * D[:, None, :]).reshape(-1, N), p + 2))
    ref.r = np.concatenate(rs)
    ref.nframes = ref.r.shape[0] // B
    ref.rows = [f.shape[0] for f in ref.feats]
    want = np.concatenate([f.reshape(-1, f.shape[1] // B) for f in ref.feats])

    def chain(r):
        a, gg = lpc_chain(r, p)
        cep = complex_cepstrum_batch(a, gg, M) if cplx else O.cepstrum_batch(a, gg, M)
        return cep, modspec_select(cep, kw["coeff_0"], M, kw["keep_even"], kw["absolute_value"], cplx)

    ref.cep, sel0 = chain(ref.r)
    ref.scale = np.maximum(1.0, np.abs(want))
    # the restated chain against the oracle's own features (the batch sums may round in another order)
    assert sel0.shape == want.shape and (np.abs(sel0 - want) / ref.scale).max() <= 1e-11
    mv = np.zeros(2)
    for seed in range(3):
        cep, sel = chain(perturbed(ref.r, seed))
        mv = np.maximum(mv, [np.abs(cep - ref.cep).max(), (np.abs(sel - sel0) / ref.scale).max()])
    ref.bar_cep, ref.bar_feat = (MARGIN * mv).tolist()
    ref.bar_env = None
    return ref


def reference(idx):
    return spectro_reference(idx) if DISPATCH_CASES[idx][6] == "spectrogram" else modspec_reference(idx)


# ---- 4. the inputs are well conditioned ------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(DISPATCH_CASES)), ids=ROW_IDS)
def test_inputs_are_well_conditioned(idx):
    ref = reference(idx)
    print("row %s: bars cep %.3g env %s feat %.3g" % (ROW_IDS[idx], ref.bar_cep,
                                                      "%.3g" % ref.bar_env if ref.bar_env else "-", ref.bar_feat))
    assert 0.0 < ref.bar_feat <= FEATURE_CAP, (ROW_IDS[idx], ref.bar_feat)


# ---- 5. GPU ------------------------------------------------------------------------------------------------
LPC_KERNELS = {"inreg": {"fdlp::lpc_env_lattice_kernel"},
               "durbin4": {"fdlp::durbin4_kernel", "fdlp::lpc_env_lattice_kernel"},
               "durbin8": {"fdlp::durbin8_kernel", "fdlp::lpc_env_lattice_kernel"},
               "lds": {"fdlp::lpc_env_kernel"}}
ALL_LPC_KERNELS = set().union(*LPC_KERNELS.values())


def run_row(row, lpc="auto", debug=False, profile=False):
    """One batch of the row's two utterances on the device: (plan, float32 rows, fp64 rows, row offsets)."""
    import torch
    from speech_recognition_tools_amd import FdlpPlan, PyRandom
    sigs = row_signals(row)
    lens = [s.size for s in sigs]
    host = FdlpPlan(feature_config(row), device=-1)
    nf = sum(host.geometry(T)[0] for T in lens)
    plan = FdlpPlan(feature_config(row), device=0, max_frames=max(16, nf))
    if row[6] != "modspec_complex":
        plan.set_lpc_path(lpc)
    if debug:
        plan.set_debug(True)
    if profile:
        plan.set_profiling(True, kernels=True)
    jit = None
    if row[6] == "spectrogram":
        jit = PyRandom(SEED).randbits2(sum(max(plan.geometry(T)[0] - 1, 0) for T in lens))
    pcm = torch.from_numpy(np.concatenate(sigs)).cuda()
    out, rows, out64 = plan.compute(pcm, lens, jit, want_f64=True)
    torch.cuda.synchronize()
    return plan, out.cpu().numpy(), out64.cpu().numpy(), rows


def row_paths(idx):
    """'auto', 'lds', and 'lattice8' where its dispatch differs from 'auto'."""
    row = DISPATCH_CASES[idx]
    paths = ["auto", "lds"]
    if host_dispatch(row, "lattice8") != host_dispatch(row, "auto"):
        paths.insert(1, "lattice8")
    return paths


def measure_row(idx):
    """Errors of every LPC path of the row against the oracle: {path: {quantity: max error}}, the fp64
    features per path and the row's bars."""
    from test_gpu_parity import durbin_errors
    row = DISPATCH_CASES[idx]
    ref = reference(idx)
    mode, B, p, M = row[6], row[1], row[4], row[5]
    res, feats = {}, {}
    for lpc in (["auto"] if mode == "modspec_complex" else row_paths(idx)):
        plan, f32, f64, rows = run_row(row, lpc, debug=mode != "modspec_complex", profile=True)
        e = {}
        want = np.concatenate(ref.feats)
        e["shape_ok"] = f64.shape == want.shape and [int(v) for v in np.diff(rows)] == [f.shape[0] for f in ref.feats]
        if mode == "spectrogram":
            e["feat"] = float(np.abs(f64 - want).max())
            e["f32"] = float(np.abs(f32 - np.round(want, 3).astype(np.float32)).max())
            e["f32_step"] = 1.0011e-3
        else:
            scale = np.maximum(1.0, np.abs(want))
            e["feat"] = float((np.abs(f64 - want) / scale).max())
            e["f32"] = float(np.abs(f32 - np.round(want, 3).astype(np.float32)).max())
            e["f32_step"] = 1.0011e-3 * float(scale.max())
        feats[lpc] = f64
        if mode != "modspec_complex":
            d = plan.debug_fetch(ref.nframes, keys=("r", "cep") + (("env",) if mode == "spectrogram" else ()))
            r = d["r"].reshape(-1, p + 2)
            e["r"] = float((np.abs(r - ref.r).max(axis=-1) / np.abs(ref.r[:, 0])).max())
            ea, eg = durbin_errors([plan], ref.nframes)
            e["items"] = int(ea.shape[1])
            e["a"], e["gg"] = float(ea.max()), float(eg.max())
            e["cep"] = float(np.abs(d["cep"].reshape(-1, M) - ref.cep).max())
            if mode == "spectrogram":
                e["env"] = float(np.abs(log_env(d["env"].reshape(ref.env.shape)) - log_env(ref.env)).max())
            disp = plan.lpc_dispatch()
            launched = set(plan.kernel_times()) & ALL_LPC_KERNELS
            e["dispatch"] = "%s%s SL%d CB%d" % (disp["durbin"][0], disp["durbin"][1] or "", disp["SL"], disp["CB"])
            e["kernels_ok"] = launched == LPC_KERNELS[disp["durbin"][0]] and disp == dict(
                host_dispatch(row, lpc), lpc_blocks=disp["lpc_blocks"]) and (disp["lpc_blocks"] > 0) == (lpc != "lds")
            e["launched"] = sorted(launched)
        res[lpc] = e
    for lpc in res:
        if lpc != "auto":
            diff = np.abs(feats[lpc] - feats["auto"])
            if mode != "spectrogram":
                diff = diff / np.maximum(1.0, np.abs(np.concatenate(ref.feats)))
            res[lpc]["feat_vs_auto"] = float(diff.max())
    bars = dict(cep=ref.bar_cep, env=ref.bar_env, feat=ref.bar_feat)
    return res, bars


def assert_row(idx):
    res, bars = measure_row(idx)
    row_id = ROW_IDS[idx]
    print("row %s bars %s" % (row_id, json.dumps(bars)))
    for lpc, e in res.items():
        print("  %-8s %s" % (lpc, json.dumps(e)))
    for lpc, e in res.items():
        what = (row_id, lpc, e.get("dispatch"))
        assert e["shape_ok"], what
        if "r" in e:
            assert e["items"] == reference(idx).r.shape[0], what
            assert e["r"] <= PERTURB, what + (e["r"],)
            assert e["a"] <= A_FLOOR and e["gg"] <= GG_FLOOR, what + (e["a"], e["gg"])
            assert e["cep"] <= bars["cep"], what + (e["cep"], bars["cep"])
            if "env" in e:
                assert e["env"] <= bars["env"], what + (e["env"], bars["env"])
            assert e["kernels_ok"], what + (e["launched"],)
        assert e["feat"] <= bars["feat"], what + (e["feat"], bars["feat"])
        assert e["f32"] <= e["f32_step"], what + (e["f32"],)
        if "feat_vs_auto" in e:
            assert e["feat_vs_auto"] <= bars["feat"], what + (e["feat_vs_auto"], bars["feat"])


@pytest.mark.gpu
@pytest.mark.parametrize("idx", SPEC_ROWS, ids=[ROW_IDS[i] for i in SPEC_ROWS])
def test_row_spectrogram(idx):
    assert_row(idx)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", MOD_ROWS, ids=[ROW_IDS[i] for i in MOD_ROWS])
def test_row_modspec(idx):
    assert_row(idx)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", CPLX_ROWS, ids=[ROW_IDS[i] for i in CPLX_ROWS])
def test_row_modspec_complex(idx):
    assert_row(idx)


# ---- the persistent grid: several item groups per resident block -----------------------------------------
GRID_CASES = [(160, 100), (135, 450), (60, 100)]  # CB 7 + durbin8, CB -1 + durbin4, CB 0 in-register
GRID_NF = 80


def measure_grid(order, M):
    """80 bands, enough 1 s utterances that every resident block of the persistent lattice kernel runs more
    than 8 item groups (the a-row prefetch 'a group ahead').  Whole batch: 'auto' against 'lds' features.
    Oracle: 8 seeded frames (debug_fetch(1, first_frame)), so the CPU side stays at seconds."""
    import torch
    from speech_recognition_tools_amd import FdlpPlan, PyRandom
    row = (COCH, GRID_NF, 0.5, 100, order, M, "spectrogram")
    cfg = feature_config(row)
    T = 16000
    probe = FdlpPlan(cfg, device=0, max_frames=16)
    blocks = probe.lpc_dispatch()["lpc_blocks"]
    fpu = probe.geometry(T)[0]
    assert blocks > 0 and fpu == 3
    n_utt = (8 * blocks * 4) // (fpu * GRID_NF) + 1   # items > 8 groups of 4 per block
    nf = n_utt * fpu
    items = nf * GRID_NF
    assert items > 8 * blocks and (items + 3) // 4 > 8 * blocks
    x = np.concatenate([speech_like(T * (n_utt // 2), 21), white(T * (n_utt - n_utt // 2), 22)])
    pcm = torch.from_numpy(x).cuda()
    jit = PyRandom(SEED).randbits2(n_utt * (fpu - 1))
    out = {}
    for lpc in ("auto", "lds"):
        plan = FdlpPlan(cfg, device=0, max_frames=nf)
        plan.set_lpc_path(lpc)
        plan.set_debug(True)
        f64 = plan.compute(pcm, [T] * n_utt, jit, want_f64=True)[2]
        torch.cuda.synchronize()
        out[lpc] = (plan, f64.cpu().numpy())
    e = dict(items=items, blocks=blocks, feat_auto_vs_lds=float(np.abs(out["auto"][1] - out["lds"][1]).max()))
    # the oracle on 8 seeded frames
    orc = O.FdlpOracle(oracle_config(row))
    frames = sorted(int(f) for f in np.random.default_rng(order).choice(nf, size=8, replace=False))
    rs = []
    for f in frames:
        u, k = divmod(f, fpu)
        fr = O.frames(x[u * T:(u + 1) * T], orc.cfg, orc.g)[k:k + 1]
        D = O.dct_frames(fr, orc.g)
        rs.append(O.autocorr_fft(orc.fbank[:, :-1] * D, order + 2))
    r = np.concatenate(rs)

    def chain(rr):
        a, gg = lpc_chain(rr, order)
        cep = O.cepstrum_batch(a, gg, M)
        return a, gg, cep, O.envelope_batch(cep * orc.w[None, :], orc.g)

    a0, gg0, cep0, env0 = chain(r)
    mv = np.zeros(2)
    for seed in range(3):
        _, _, cep, env = chain(perturbed(r, seed))
        mv = np.maximum(mv, [np.abs(cep - cep0).max(), np.abs(log_env(env) - log_env(env0)).max()])
    bars = dict(cep=MARGIN * mv[0], env=MARGIN * mv[1], feat=FEATURE_CAP)
    for lpc, (plan, _) in out.items():
        keys = ("r", "a", "gg", "cep", "env")
        got = [plan.debug_fetch(1, f, keys=keys) for f in frames]
        d = {k: np.concatenate([g[k].reshape(GRID_NF, -1) for g in got]) for k in keys}
        e[lpc] = dict(r=float((np.abs(d["r"] - r).max(axis=-1) / r[:, 0]).max()),
                      cep=float(np.abs(d["cep"] - cep0).max()),
                      env=float(np.abs(log_env(d["env"]) - log_env(env0)).max()))
        # a / gg against solve_toeplitz on the device's own r
        ad, ggd = lpc_chain(d["r"], order)
        e[lpc]["a"] = float((np.abs(d["a"] - ad).max(axis=-1) / np.abs(ad).max(axis=-1)).max())
        e[lpc]["gg"] = float((np.abs(d["gg"][:, 0] - ggd) / np.abs(ggd)).max())
    return e, bars


@pytest.mark.gpu
@pytest.mark.parametrize("order,M", GRID_CASES)
def test_persistent_grid_runs_many_groups_per_block(order, M):
    e, bars = measure_grid(order, M)
    print("grid p%d M%d: %s bars %s" % (order, M, json.dumps(e), json.dumps(bars)))
    # the whole batch has no oracle (the CPU side stays at seconds): the two paths are held to the cap every
    # row's feature bar obeys; the sampled frames to bars from their own conditioning
    assert e["feat_auto_vs_lds"] <= bars["feat"]
    for lpc in ("auto", "lds"):
        m = e[lpc]
        assert m["r"] <= PERTURB and m["a"] <= A_FLOOR and m["gg"] <= GG_FLOOR, (lpc, m)
        assert m["cep"] <= bars["cep"] and m["env"] <= bars["env"], (lpc, m, bars)


# ---- the range-check build -----------------------------------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import torch
import test_lpc_dispatch as T
from speech_recognition_tools_amd.plan import device_checks
assert device_checks(reset=True)[0], "not a checks build"
runs = 0
for row in T.DISPATCH_CASES:
    T.run_row(row)
    runs += 1
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": runs}))
"""


@pytest.mark.gpu
def test_rows_under_range_checks():
    """Every row once through the library built with -DFDLP_DEVICE_CHECKS=1 (one child process: the library
    is chosen when it is loaded): the lattice kernel's la / cs image for every CB, the sliding window of the
    CB -1 cepstrum, the LDS-DMA a rows, the envelope's cosine-table index and cplx_lpc_out_kernel's ys / a /
    cep stay inside their ranges.  The table index is the only place the `u % env_nfft` of the envelope setup
    can show: the lanes it changes (u > env_nfft / 4) emit nothing, so no output depends on it."""
    assert os.path.exists(CHECKS_LIB), "build() compiles libfdlp_checks.so"
    env = dict(os.environ, FDLP_LIB=CHECKS_LIB)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["enabled"] and res["runs"] == len(DISPATCH_CASES)
    assert res["violations"] == 0, res


# ---- 6. the recorded measurements ------------------------------------------------------------------------
def worst_ratios(records):
    """{quantity: (error / bar, row, path)} over recorded rows; a and gg against their floors."""
    worst = {}
    for rec in records:
        for lpc, e in rec["paths"].items():
            for q, bar in (("a", A_FLOOR), ("gg", GG_FLOOR), ("r", PERTURB), ("cep", rec["bars"]["cep"]),
                           ("env", rec["bars"].get("env")), ("feat", rec["bars"]["feat"])):
                if q in e and bar:
                    ratio = e[q] / bar
                    if ratio > worst.get(q, (0.0,))[0]:
                        worst[q] = (float("%.3g" % ratio), rec["row"], lpc)
    return worst


def test_recorded_errors_match_docstring():
    """tests/data/lpc_dispatch_errors.jsonl holds one record per row and grid case, every recorded error is
    within its bar, and MEASURED_WORST quotes that file's worst ratios."""
    assert os.path.exists(ERRORS_FILE)
    recs = [json.loads(l) for l in open(ERRORS_FILE)]
    rows = [r for r in recs if "paths" in r]
    assert [r["row"] for r in rows] == ROW_IDS
    assert len([r for r in recs if "grid" in r]) == len(GRID_CASES)
    worst = worst_ratios(rows)
    assert all(v[0] <= 1.0 for v in worst.values()), worst
    assert {k: tuple(v) for k, v in worst.items()} == MEASURED_WORST


def record(path=ERRORS_FILE):
    with open(path, "w") as f:
        for idx in range(len(DISPATCH_CASES)):
            res, bars = measure_row(idx)
            f.write(json.dumps(dict(row=ROW_IDS[idx], bars=bars, paths=res)) + "\n")
            f.flush()
        for order, M in GRID_CASES:
            e, bars = measure_grid(order, M)
            f.write(json.dumps(dict(grid=[order, M], bars=bars, errors=e)) + "\n")
            f.flush()
    recs = [json.loads(l) for l in open(path)]
    print("MEASURED_WORST = %r" % ({k: tuple(v) for k, v in worst_ratios([r for r in recs if "paths" in r]).items()},))


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_lpc_dispatch.py --record [file]")
    rest = [a for a in sys.argv[1:] if a != "--record"]
    record(rest[0] if rest else ERRORS_FILE)
