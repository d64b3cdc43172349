"""The block schedule of the lag-parallel VALU sweeps (ac_vsweep_kernel): runs of whole blocks taken without
a test, between the general blocks that hold events, sweep ends and chunk commits.

The schedule depends on the plan alone.  plan.sweep_schedule() replays the kernel's walk on the host with the
kernel's own run rule (vs_plain_low, fdlp_internal.h), so it is checked here without a device, against
plan.regions() and plan.flat_events(): every position of [nlo, nhi) is consumed exactly once, a run holds no
event, no sweep end and nothing that is not staged, every event is handled in the block that holds it, run
counts are even (the window banks alternate).  An event exactly at a block's base n0 is handled at the head of
the block below (or at the sweep's end): nothing is consumed in between, and so it was before the runs.

Shapes: the three lag widths of test_vsweep_block_order.py, the p = 238 shape of
test_structured_autocorr_matches_oracle (240 lags: no VALU sweeps, hence no schedule; the MFMA sweeps run), the
shortest frame a plan accepts (fduration 0.064 s, N = 1024), and two one-band banks whose sweeps are shorter
than one 256-position chunk: at the shortest frame a flat sweep of a few positions (less than two blocks, its
top block cut by the sweep's top) beside an empty lower-skirt sweep (the single END record), and at the
recipes' frame and order a flat sweep of 151 positions that takes one run between its two ends, with
nothing below to commit.

On the GPU the same shapes at 1, 3 and 5 frames against the oracle's FFT autocorrelation, at the bar of
test_vsweep_block_order.py: max over lags of |dr| / r[0] <= 1e-12."""
import functools

import numpy as np
import pytest

# (fbank_type, nfilters, fduration, order, coeff_num)
SHAPES = {
    "a4": ("cochlear,2,0.5,1,4,1.2", 20, 0.5, 20, 20),
    "a8": ("cochlear,0.02,1,1,2.5,1", 30, 0.5, 100, 40),
    "a10": ("cochlear,1,1,1,2.5,1", 80, 1.5, 150, 100),
    "p238": ("cochlear,1,1,1,2.5,1", 7, 1.5, 238, 100),
    "short": ("cochlear,1,1,1,2.5,1", 5, 0.064, 10, 10),
    "one": ("cochlear,1,1,1,2.5,1", 1, 0.064, 10, 10),
    "one150": ("cochlear,1,1,1,2.5,1", 1, 1.5, 150, 100),
}
COMMIT, GENERAL, END = 0, 1, 2
RING = 512
TOL = 1e-12


def _cfg(tag):
    from speech_recognition_tools_amd import FeatureConfig
    fb, nf, fd, order, cn = SHAPES[tag]
    return FeatureConfig(fbank_type=fb, nfilters=nf, fduration=fd, order=order, coeff_num=cn,
                         coeff_range="0,%d" % cn)


@functools.lru_cache(maxsize=None)
def _sweeps(tag):
    """[(name, info, events S in sweep order, records)] of a host-only plan's sweeps."""
    from speech_recognition_tools_amd import FdlpPlan
    plan = FdlpPlan(_cfg(tag), device=-1, max_frames=64)
    chains, parts, ev = plan.flat_events()
    if chains == 0:
        for kind in (0, 1):
            assert len(plan.sweep_schedule(kind)[1]) == 0
        return []
    m1, m2 = plan.regions()
    out = []
    for kind, S in ((0, plan.N - m1.astype(np.int64)), (1, m2.astype(np.int64))):
        info, rec = plan.sweep_schedule(kind)
        assert info["nhi"] == plan.N and info["nlo"] == S.min()
        out.append(("skirt%d" % kind, info, np.sort(S)[::-1], rec))
    k = 0
    for h in range(parts):  # part h takes the events at or above its lower end, the last part the rest
        info, rec = plan.sweep_schedule(2, h)
        k1 = len(ev) if h == parts - 1 else k + int((ev[k:, 0] >= info["nlo"]).sum())
        assert np.all(np.diff(ev[:, 0]) <= 0)
        out.append(("flat%d" % h, info, ev[k:k1, 0].astype(np.int64), rec))
        k = k1
    return out


def _replay(info, S, rec):
    """Walks one schedule; returns the cases it met."""
    A, chunk, nlo, nhi = info["A"], info["chunk"], info["nlo"], info["nhi"]
    assert A in (4, 8, 10) and chunk in (128, 256)
    if nhi <= nlo:  # nothing to sweep: every row is zero
        assert rec.tolist() == [[0, END, nlo, len(S)]]
        return {"empty sweep"}
    assert rec[-1][1] == END and not np.any(rec[:-1, 1] == END)
    b_top, b_bot = (nhi - 1) // A, nlo // A
    consumed = np.zeros(nhi + A, dtype=np.int64)
    staged = None  # first staged position
    b, k = b_top, 0
    met = set()
    prev = None  # (action, aux) of the previous record

    def resident(n0):
        # the block's window, and the broadcast source of the block below it
        assert staged is not None and max(n0 - A, A * b_bot) >= staged and n0 + 16 * A <= staged + RING, (n0, staged)

    for run, action, pos, aux in rec.tolist():
        assert run % 2 == 0 and run >= 0
        for _ in range(run):
            n0 = A * b
            assert nlo <= n0 and n0 + A <= nhi, "a run holds a sweep end"
            assert k == len(S) or S[k] < n0, "a run holds an event"
            assert n0 > A * b_bot
            resident(n0)
            consumed[n0:n0 + A] += 1
            b -= 1
        if action == COMMIT:
            assert pos % chunk == 0 and (staged is None or pos == staged - chunk)
            staged = pos
        elif action == GENERAL:
            n0 = A * b
            assert pos == n0 and b >= b_bot
            resident(n0)
            consumed[max(n0, nlo):min(n0 + A, nhi)] += 1
            here = S[k:k + aux]
            assert len(here) == aux
            for s in here:  # in this block, its top boundary included; at or past the sweep's top in the top block
                assert n0 < s <= n0 + A or (b == b_top and s >= nhi), (s, n0)
            k += aux
            # (an event at the sweep's lower end waits for the end of the sweep, like one at the block's base)
            assert k == len(S) or S[k] <= max(n0, nlo), "an event of this block is left behind"
            if aux >= 2 and len(set(here.tolist())) >= 2:
                met.add("two events in one block")
            if aux and run == 0 and prev == (GENERAL, True):
                met.add("events in adjacent blocks")
            if aux and prev is not None and prev[0] == COMMIT:
                met.add("event block at a chunk boundary")
            if aux and b == b_top:
                met.add("event in the first block")
            if aux and b == b_bot:
                met.add("event in the last block")
            b -= 1
        else:
            assert b == b_bot - 1 and aux == len(S) - k
            assert np.all(S[k:] <= max(nlo, A * b_bot))  # everything at or above them is consumed
            if aux and np.any(S[k:] >= A * b_bot):
                met.add("event in the last block")
            k += aux
        prev = (action, bool(aux))
    assert k == len(S)
    assert np.all(consumed[nlo:nhi] == 1) and consumed[:nlo].sum() == 0 and consumed[nhi:].sum() == 0
    if rec[:, 0].max() > 0:
        met.add("runs")
    if nhi - nlo < 256:  # shorter than one chunk of either sweep kind
        met.add("short sweep")
        if rec[:, 0].max() > 0:
            met.add("short sweep with a run")
            assert not np.any(rec[np.argmax(rec[:, 0] > 0):, 1] == COMMIT), "nothing is left to commit below the run"
        if nhi - nlo < 2 * A and nhi % A:
            met.add("sweep of less than two blocks, top block cut")
    return met


@pytest.mark.parametrize("tag", list(SHAPES))
def test_schedule_replay(tag):
    sweeps = _sweeps(tag)
    if tag == "p238":
        assert sweeps == []  # 240 lags: the plan keeps the MFMA sweeps
        return
    assert len(sweeps) >= 3
    for name, info, S, rec in sweeps:
        met = _replay(info, S, rec)
        print(tag, name, info, "records", len(rec), "blocks in runs", int(rec[:, 0].sum()), sorted(met))
        assert "runs" in met or info["nhi"] - info["nlo"] < 512


def test_cases_occur():
    """Between them the shapes hold every case the general block exists for."""
    met = set()
    for tag in SHAPES:
        for _, info, S, rec in _sweeps(tag):
            met |= _replay(info, S, rec)
    want = {"two events in one block", "events in adjacent blocks", "event in the first block",
            "event in the last block", "event block at a chunk boundary", "runs", "empty sweep", "short sweep",
            "short sweep with a run", "sweep of less than two blocks, top block cut"}
    assert want <= met, want - met


def test_shortest_frame_and_shortest_sweeps():
    """fduration 0.064 s is the shortest frame a plan accepts (1024 samples); the one-band shapes' sweeps are
    shorter than one chunk."""
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig
    from speech_recognition_tools_amd._lib import FdlpError
    fb, nf, fd, order, cn = SHAPES["short"]
    assert FdlpPlan(_cfg("short"), device=-1, max_frames=64).N == 1024
    for tag, want in (("one", (1, 2 * 4)), ("one150", (128, 256))):
        flat = [info["nhi"] - info["nlo"] for name, info, _, _ in _sweeps(tag) if name.startswith("flat")]
        print(tag, "flat sweep positions", flat)
        assert len(flat) == 1 and want[0] <= flat[0] < want[1], (tag, flat)
    assert any(info["nhi"] <= info["nlo"] for _, info, _, _ in _sweeps("one"))
    with pytest.raises(FdlpError, match="1024 samples"):
        FdlpPlan(FeatureConfig(fbank_type=fb, nfilters=nf, fduration=1023 / 16000.0, order=order, coeff_num=cn,
                               coeff_range="0,%d" % cn), device=-1, max_frames=64)


@functools.lru_cache(maxsize=None)
def _gpu_plan(tag):
    from speech_recognition_tools_amd import FdlpPlan
    plan = FdlpPlan(_cfg(tag), device=0, max_frames=64)
    assert plan.autocorr_path == ("structured_mfma" if tag == "p238" else "structured")
    plan.set_debug(True)
    return plan


def _length_for_frames(plan, F):
    for T in range(50, 16000 * 40, 50):
        if plan.geometry(T)[0] == F:
            return T
    raise AssertionError("no utterance length gives %d frames" % F)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 3, 5])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_sweeps_match_oracle(tag, F):
    import torch

    from oracle import fdlp_oracle as O
    from speech_recognition_tools_amd import PyRandom
    plan = _gpu_plan(tag)
    fb, nf, fd, order, cn = SHAPES[tag]
    ocfg = O.FdlpConfig(fbank_type=fb, nfilters=nf, fduration=fd, order=order, coeff_num=cn,
                        coeff_range="0,%d" % cn)
    T = _length_for_frames(plan, F)
    rng = np.random.default_rng(100 * F + nf)
    t = np.arange(T) / 16000.0
    speechy = (3000 * np.sin(2 * np.pi * 180 * t) * (1 + np.sin(2 * np.pi * 3 * t))
               + 200 * rng.standard_normal(T)).astype(np.int16)
    white = (rng.standard_normal(T) * 8000).astype(np.int16)
    for name, x in (("speech", speechy), ("white", white)):
        keep = O.Intermediates()
        O.FdlpOracle(ocfg).band_envelopes(x, keep)
        assert keep.r.shape[0] == F
        plan.compute(torch.from_numpy(x).cuda(), [T], PyRandom(0).randbits2(F - 1))
        torch.cuda.synchronize()
        got = plan.debug_fetch(F, keys=("r",))["r"]
        rel = (np.abs(got - keep.r) / np.abs(keep.r[..., :1])).max()
        print(tag, F, name, "rel", rel)
        assert rel <= TOL, (name, rel)
