"""The lag-parallel VALU sweeps (ac_vsweep_kernel) against the oracle's FFT autocorrelation on shapes
chosen for the order in which a block issues its FMAs and for the event path: the three lag widths
(A = 4, 8, 10 lags per lane), events at every residue of S mod A, two events inside one block (the
masked two-pass path), and frame counts that leave invalid rows in the last group of four.

Bar: max over lags of |dr| / r[0] <= 1e-12, the bar of test_structured_autocorr_matches_oracle; the
VALU and the MFMA sweeps, each within that bar, agree with each other to 2e-12."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (fbank_type, nfilters, fduration, order, coeff_num, lags per lane)
CFGS = {
    "a4": ("cochlear,2,0.5,1,4,1.2", 20, 0.5, 20, 20, 4),
    "a8": ("cochlear,0.02,1,1,2.5,1", 30, 0.5, 100, 40, 8),     # near-empty flat tops
    "a10": ("cochlear,1,1,1,2.5,1", 80, 1.5, 150, 100, 10),     # the recipes' shape
}
FRAMES = [1, 2, 3, 5, 9]
TOL = 1e-12


@functools.lru_cache(maxsize=None)
def _plan(tag):
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig
    fb, nf, fd, order, cn, _ = CFGS[tag]
    cfg = FeatureConfig(fbank_type=fb, nfilters=nf, fduration=fd, order=order, coeff_num=cn,
                        coeff_range="0,%d" % cn)
    plan = FdlpPlan(cfg, device=0, max_frames=64)
    assert plan.autocorr_path in ("structured", "structured_mfma")
    plan.set_debug(True)
    return plan


def _oracle_cfg(tag):
    from oracle import fdlp_oracle as O
    fb, nf, fd, order, cn, _ = CFGS[tag]
    return O.FdlpConfig(fbank_type=fb, nfilters=nf, fduration=fd, order=order, coeff_num=cn,
                        coeff_range="0,%d" % cn)


def _event_positions(plan):
    """Sweep positions of every event of the three sweeps: lower-skirt snapshots at N - m1_j, upper-skirt
    snapshots at m2_j, flat-top restarts and emissions as the plan lists them."""
    m1, m2 = plan.regions()
    chains, _, ev = plan.flat_events()
    assert chains > 0, "the plan has no VALU sweeps"
    return (plan.N - m1).astype(np.int64), m2.astype(np.int64), ev[:, 0].astype(np.int64)


def _length_for_frames(plan, F):
    """The shortest utterance (in steps of 50 samples) that the plan cuts into F frames."""
    for T in range(50, 16000 * 40, 50):
        if plan.geometry(T)[0] == F:
            return T
    raise AssertionError("no utterance length gives %d frames" % F)


def test_lags_per_lane():
    """The three shapes run the three instantiations: the smallest of 4, 8, 10 that holds nlags / 16."""
    for tag, c in CFGS.items():
        a = (_plan(tag).nlags + 15) // 16
        assert min(v for v in (4, 8, 10) if a <= v) == c[5], tag


def test_events_cover_every_residue():
    """The 80-band shape has an event at every residue of S mod A in each of its sweeps' union."""
    plan = _plan("a10")
    A = CFGS["a10"][5]
    S = np.concatenate(_event_positions(plan))
    print("residues", np.bincount(S % A, minlength=A))
    assert set((S % A).tolist()) == set(range(A))


def test_two_events_in_one_block():
    """The near-empty flat tops put a restart and an emission into one block of A positions."""
    plan = _plan("a8")
    A = CFGS["a8"][5]
    flat = _event_positions(plan)[2]
    blocks, n = np.unique(flat // A, return_counts=True)
    print("flat events", flat.size, "blocks with two or more", int((n >= 2).sum()))
    assert (n >= 2).any()


@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("tag", list(CFGS))
def test_sweeps_match_oracle(tag, F):
    from oracle import fdlp_oracle as O
    from speech_recognition_tools_amd import PyRandom
    plan = _plan(tag)
    T = _length_for_frames(plan, F)
    rng = np.random.default_rng(1000 * F + CFGS[tag][5])
    t = np.arange(T) / 16000.0
    speechy = (3000 * np.sin(2 * np.pi * 180 * t) * (1 + np.sin(2 * np.pi * 3 * t))
               + 200 * rng.standard_normal(T)).astype(np.int16)
    white = (rng.standard_normal(T) * 8000).astype(np.int16)
    try:
        for name, x in (("speech", speechy), ("white", white)):
            keep = O.Intermediates()
            O.FdlpOracle(_oracle_cfg(tag)).band_envelopes(x, keep)
            assert keep.r.shape[0] == F
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
