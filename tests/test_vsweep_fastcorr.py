"""The lag-parallel VALU sweeps with their plain runs in the 2x2 fast-correlation form (ac_vsweep_kernel,
vs_fast22) against the oracle's FFT autocorrelation, on inputs chosen for the sums that form adds: it multiplies
differences of neighbouring window elements and sums of neighbouring positions, so the inputs are

  impulse      one full-scale sample per frame: the DCT is a few cosines, a line spectrum after the utterance's
               reflection; most neighbouring differences and sums are differences of nearly equal numbers
  alternating  full-scale +a, -a, +a, ...: all energy at the top of the DCT, ~100 dB above the rest of it
  lsb          noise of 1 LSB amplitude (values -1, 0, 1): scale

Shapes: the three lag widths of test_vsweep_block_order.py (A = 4, 8, 10 lags per lane) at F = 1 (a last group of
four with three invalid rows) and F = 5 (two groups), max_frames = 64.  The skirt sweeps <A, 0> take the 2x2 form
at all three widths; the flat sweep takes it at a4 (<4, 4>) and a10 (<10, 5>) only: the a8 row needs one chain and
runs <8, 4>, which vs_fast22 leaves in the direct form.  The 2x2 form in the flat sweep at A = 8 (<8, 5>, <8, 6>,
<8, 8>) is held by rows 5, 8 and 11 of test_autocorr_dispatch.py, on the same inputs.

Bar: max over lags of |dr| / r[0] <= 1e-12, the project's; the VALU and the MFMA sweeps agree to 2e-12.  The bar
presumes that the oracle's own r is far inside it for these inputs: test_oracle_is_inside_the_bar holds it, at
F = 1, against a direct long-double sum over the same band signals (measured 2e-16 .. 5e-16 at F = 1 and
3e-16 .. 8e-16 at F = 5 for all nine shape x input pairs, so all three inputs are kept).

Measured on MI355X: impulse and lsb 4e-16 .. 1.4e-14 on either sweep form; alternating 9.6e-14 (a4), 8.8e-13 (a8),
3.6e-13 (a10), the same on the VALU and the MFMA sweeps (what is upstream of them, at ~100 dB of spectral range);
the two sweep forms agree to <= 1.3e-15 on every case."""
import functools

import numpy as np
import pytest

# (fbank_type, nfilters, fduration, order, coeff_num, lags per lane)
CFGS = {
    "a4": ("cochlear,2,0.5,1,4,1.2", 20, 0.5, 20, 20, 4),
    "a8": ("cochlear,0.02,1,1,2.5,1", 30, 0.5, 100, 40, 8),
    "a10": ("cochlear,1,1,1,2.5,1", 80, 1.5, 150, 100, 10),
}
INPUTS = ("impulse", "alternating", "lsb")
TOL = 1e-12
# the oracle against long double: the rounding of its FFT pair, of the order of eps log2(N) = 1.1e-16 x 14.6 =
# 1.6e-15 of r[0] for N = 24000; a hundredth of the bar, which then belongs to the kernel
ORACLE_TOL = 1e-14


def _cfgs(tag):
    from oracle import fdlp_oracle as O
    from speech_recognition_tools_amd import FeatureConfig
    fb, nf, fd, order, cn, _ = CFGS[tag]
    kw = dict(fbank_type=fb, nfilters=nf, fduration=fd, order=order, coeff_num=cn, coeff_range="0,%d" % cn)
    return FeatureConfig(**kw), O.FdlpConfig(**kw)


@functools.lru_cache(maxsize=None)
def _host_plan(tag):
    from speech_recognition_tools_amd import FdlpPlan
    return FdlpPlan(_cfgs(tag)[0], device=-1, max_frames=64)


@functools.lru_cache(maxsize=None)
def _length_for_frames(tag, F):
    """The shortest utterance (in steps of 50 samples) that the plan cuts into F frames."""
    plan = _host_plan(tag)
    for T in range(50, 16000 * 40, 50):
        if plan.geometry(T)[0] == F:
            return T
    raise AssertionError("no utterance length gives %d frames" % F)


def _signal(name, T, F):
    if name == "impulse":
        x = np.zeros(T, dtype=np.int16)
        x[[int(T * (2 * i + 1) / (2 * F)) for i in range(F)]] = 32767
        return x
    if name == "alternating":
        return (32767 * (1 - 2 * (np.arange(T) % 2))).astype(np.int16)
    return np.random.default_rng(7).integers(-1, 2, size=T).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _oracle(tag, F, name):
    """(x, T, the oracle's intermediates), computed once per case and left unchanged."""
    from oracle import fdlp_oracle as O
    T = _length_for_frames(tag, F)
    x = _signal(name, T, F)
    keep = O.Intermediates()
    orc = O.FdlpOracle(_cfgs(tag)[1])
    orc.band_envelopes(x, keep)
    assert keep.r.shape[0] == F and np.abs(keep.r[..., 0]).min() > 0
    keep.r.setflags(write=False)
    return x, T, keep, orc.fbank


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("tag", list(CFGS))
def test_oracle_is_inside_the_bar(tag, name):
    """The oracle's circular FFT autocorrelation against the same sum in long double over the same band signals."""
    x, T, keep, fbank = _oracle(tag, 1, name)
    bands = (fbank[None, :, :-1] * keep.dct[:, None, :]).reshape(-1, keep.dct.shape[-1]).astype(np.longdouble)
    r = keep.r.reshape(bands.shape[0], -1)
    ref = np.stack([(bands * np.roll(bands, -lag, axis=1)).sum(axis=1) for lag in range(r.shape[1])], axis=1)
    rel = float((np.abs(r - ref) / np.abs(r[:, :1])).max())
    print(tag, name, "oracle against long double", rel)
    assert rel <= ORACLE_TOL, rel


@functools.lru_cache(maxsize=None)
def _plan(tag):
    from speech_recognition_tools_amd import FdlpPlan
    plan = FdlpPlan(_cfgs(tag)[0], device=0, max_frames=64)
    assert plan.autocorr_path in ("structured", "structured_mfma")
    a = (plan.nlags + 15) // 16
    assert min(v for v in (4, 8, 10) if a <= v) == CFGS[tag][5]
    plan.set_debug(True)
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("tag", list(CFGS))
def test_fastcorr_sweeps_match_oracle(tag, F):
    import torch

    from speech_recognition_tools_amd import PyRandom
    plan = _plan(tag)
    try:
        for name in INPUTS:
            x, T, keep, _ = _oracle(tag, F, name)
            scale = np.abs(keep.r[..., :1])
            got = {}
            for path in ("structured", "structured_mfma"):
                plan.set_autocorr_path(path)
                plan.compute(torch.from_numpy(x).cuda(), [T], PyRandom(0).randbits2(F - 1))
                torch.cuda.synchronize()
                got[path] = plan.debug_fetch(F, keys=("r",))["r"]
                rel = (np.abs(got[path] - keep.r) / scale).max()
                print(tag, F, name, path, "rel", rel)
                assert rel <= TOL, (name, path, rel)
            cross = (np.abs(got["structured"] - got["structured_mfma"]) / scale).max()
            print(tag, F, name, "cross", cross)
            assert cross <= 2 * TOL, (name, cross)
    finally:
        plan.set_autocorr_path("auto")
