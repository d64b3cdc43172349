"""Every kernel instantiation the structured autocorrelation can dispatch to, against the CPU oracle.

launch_vsweep_a (csrc/fdlp_autocorr.hip) picks ac_vsweep_kernel<A, C> for the flat tops from the lags per lane
A in {4, 8, 10} (vsweep_lanes_lags) and the chain slots C in {4, 5, 6, 8} (vsweep_chains), the flat sweep runs as
1 or 2 position parts, vs_fast22<A, C>() decides whether an instantiation takes its plain runs in the 2x2
fast-correlation form, ac_wrap_kernel runs or not, ac_band_kernel stages a band's straddles in its compact `fast`
form or in the general one, and plans the VALU sweeps do not fit fall back to the MFMA sweeps or to the direct
kernel.  DISPATCH_ROWS holds one small plan (N <= 8000, at most 24 bands) per instantiation and branch:

* test_rows_reach_their_instantiation, test_table_covers_dispatch_space (CPU): FdlpPlan.autocorr_dispatch() of
  host-only plans reaches, over the table, every <A, C> with every slot in use and two parts, both plain-run forms
  at every A that has both, one part at every C, an idle chain slot, ac_wrap_kernel on and off, bands on both sides
  of the `fast` staging and the three default paths; per A some row has two flat events in one block of A
  positions and flat events at every residue of S mod A.  A changed threshold (vsweep_chains, vs_fast22, the 2048
  positions of flat_parts, ...) fails here until the table follows it.
* test_edge_rows_have_their_edges (CPU): the rows named for an edge have it (a lower-skirt sweep with nothing to
  sweep, an upper-skirt snapshot at N, flat tops of width 0, the last order with VALU sweeps).
* test_oracle_is_inside_the_bar (CPU): at F = 1 the oracle's FFT autocorrelation of every row and input against a
  long-double direct circular sum over the same band signals, within ORACLE_TOL = 1e-14 of r[0].
* test_row (GPU): five inputs (speech-like, white, impulse, alternating, lsb) x three batches (F = 1: three invalid
  rows in the group of four; F = 5: two groups; two utterances of 2 + 4 frames: a group across the utterance
  boundary) x every path the row has.  The device r against the oracle's FFT autocorrelation of fbank x the
  device's own dct ("own": the bar belongs to this stage alone) and against the oracle's r from the PCM ("e2e"),
  max over lags of |dr| / r[0] <= 1e-12 (e2e of `alternating` is printed and recorded, not asserted: its ~100 dB
  of spectral range shows what is upstream of the sweeps, see test_vsweep_fastcorr.py); 'structured' and
  'structured_mfma' agree to 2e-12; kernel_times() shows exactly the kernels autocorr_dispatch() names.
* test_rows_under_range_checks (GPU): every row once at F = 5 under the range-check build, zero violations.

`python tests/test_autocorr_dispatch.py --record` (on the device) rewrites tests/data/autocorr_dispatch_errors.jsonl,
one record per row with the maxima of every input, batch and path.  MEASURED_WORST below quotes that file's worst
values (of r[0]; the bar is 1e-12): own 4.0e-14 (row 14, alternating, 2 + 4 frames, on 'structured_mfma'; 1e-15 ..
8e-15 on every row of N = 8000 but row 21), e2e of the asserted inputs 2.5e-14 (row 21, nlags = 160, speech at F = 5
on 'structured', which is also the largest distance between the two structured paths, 2.5e-14), e2e of alternating
8.8e-13 (row 20 at F = 1, the same on both paths: what is upstream of the sweeps, as in test_vsweep_fastcorr.py);
test_recorded_errors_match_docstring keeps the two equal.  Every instantiation sits a factor 25 or more inside the
bar on its own input: no row failed and no kernel changed.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import fdlp_oracle as O

C1 = "cochlear,1,1,1,2.5,1"
C7 = "cochlear,7,1,1,2.5,1"     # wide flat tops: many of them overlap, so the flat sweep needs many chains
C8 = "cochlear,8,1,1,2.5,1"
COEFF_NUM = 10
MAX_FRAMES = 64
TOL = 1e-12          # of r[0]: the project's bar on the device autocorrelation
ORACLE_TOL = 1e-14   # the oracle against long double (test_vsweep_fastcorr.py: eps log2(N), a hundredth of TOL)
ERRORS_FILE = os.path.join(ROOT, "tests", "data", "autocorr_dispatch_errors.jsonl")
CHECKS_LIB = os.path.join(ROOT, "speech_recognition_tools_amd", "lib", "libfdlp_checks.so")

# Worst recorded value per quantity over tests/data/autocorr_dispatch_errors.jsonl as (value, row, case);
# test_recorded_errors_match_docstring compares them with the file.
MEASURED_WORST = {
    "own": (4.01e-14, "14-8_1_1_2.5_1-B20-fd0.1-p150", "alternating/F2+4/structured_mfma"),
    "e2e": (2.54e-14, "21-1_1_1_2.5_1-B10-fd0.5-p158", "speech/F5/structured"),
    "e2e_alternating": (8.77e-13, "20-0.0001_1_1_2.5_1-B10-fd0.5-p20", "alternating/F1/structured"),
    "cross": (2.54e-14, "21-1_1_1_2.5_1-B10-fd0.5-p158", "speech/F5"),
}


def _vs(A, C, chains, parts):
    return dict(path="structured", lanes_lags=A, chain_slots=C, chains=chains, parts=parts)


# (fbank_type, nfilters, fduration, order, what 'auto' launches); N = 16000 fduration
DISPATCH_ROWS = [
    # ---- every <A, C> with all C chains in use and two position parts ----
    (C7, 10, 0.5, 20, _vs(4, 4, 4, 2)),
    (C7, 10, 0.5, 100, _vs(8, 4, 4, 2)),       # the one A = 8 instantiation with plain runs in the direct form
    (C7, 10, 0.5, 150, _vs(10, 4, 4, 2)),
    (C8, 12, 0.5, 20, _vs(4, 5, 5, 2)),
    (C8, 12, 0.5, 100, _vs(8, 5, 5, 2)),       # A = 8 in the 2x2 form
    (C8, 12, 0.5, 150, _vs(10, 5, 5, 2)),
    (C7, 16, 0.5, 20, _vs(4, 6, 6, 2)),
    (C7, 16, 0.5, 100, _vs(8, 6, 6, 2)),
    (C7, 16, 0.5, 150, _vs(10, 6, 6, 2)),      # A = 10 with plain runs in the direct form
    (C8, 20, 0.5, 20, _vs(4, 8, 8, 2)),
    (C8, 20, 0.5, 100, _vs(8, 8, 8, 2)),
    (C8, 20, 0.5, 150, _vs(10, 8, 8, 2)),
    # ---- an idle chain slot, one position part, the smallest frame ----
    (C8, 16, 0.5, 150, _vs(10, 8, 7, 2)),
    (C8, 20, 0.1, 150, _vs(10, 8, 8, 1)),
    (C7, 16, 0.1, 100, _vs(8, 6, 6, 1)),
    (C8, 20, 0.064, 150, _vs(10, 8, 8, 1)),    # N = 1024, the plan's minimum
    (C8, 12, 0.1, 20, _vs(4, 5, 5, 1)),
    # ---- edges of the sweeps ----
    (C1, 1, 0.5, 20, _vs(4, 4, 1, 1)),         # one band, m1 = 0: the lower-skirt sweep has nhi <= nlo
    (C1, 2, 0.5, 20, _vs(4, 4, 1, 2)),         # the last band's m2 = N: an upper-skirt snapshot at the very top
    ("cochlear,0.0001,1,1,2.5,1", 10, 0.5, 20, _vs(4, 4, 1, 2)),   # flat tops of width 0 and 1
    (C1, 10, 0.5, 158, _vs(10, 4, 1, 2)),      # nlags = 160, the last order with VALU sweeps
    # ---- fallbacks ----
    (C1, 10, 0.5, 159, dict(path="structured_mfma")),              # nlags = 161
    (C7, 24, 0.5, 100, dict(path="structured_mfma")),              # more than 8 chains
    ("cochlear,1,1,0,2.5,1", 10, 0.5, 20, dict(path="direct")),    # fixed = 0: no skirt factorisation
    ("cochlear,1,7,1,2.5,1", 10, 0.5, 20, dict(path="direct")),    # skirt exponent over the table's limit
]
NROWS = len(DISPATCH_ROWS)
ROW_IDS = ["%02d-%s-B%d-fd%g-p%d" % (i + 1, r[0].split(",", 1)[1].replace(",", "_"), r[1], r[2], r[3])
           for i, r in enumerate(DISPATCH_ROWS)]
VS_ROWS = [i for i, r in enumerate(DISPATCH_ROWS) if r[4]["path"] == "structured"]
INPUTS = ("speech", "white", "impulse", "alternating", "lsb")
BATCHES = {"F1": (1,), "F5": (5,), "F2+4": (2, 4)}   # frames per utterance
E2E_ASSERTED = ("speech", "white", "impulse", "lsb")
# the launcher's two switches (launch_vsweep, launch_vsweep_a) and which <A, C> have which plain-run form
ALL_A, ALL_C = (4, 8, 10), (4, 5, 6, 8)
FAST22_FORMS = {4: {True}, 8: {False, True}, 10: {False, True}}


def _cfgs(idx):
    from speech_recognition_tools_amd import FeatureConfig
    fb, nf, fd, order, _ = DISPATCH_ROWS[idx]
    kw = dict(fbank_type=fb, nfilters=nf, fduration=fd, order=order, coeff_num=COEFF_NUM,
              coeff_range="0,%d" % COEFF_NUM)
    return FeatureConfig(**kw), O.FdlpConfig(**kw)


@functools.lru_cache(maxsize=None)
def _host_plan(idx):
    from speech_recognition_tools_amd import FdlpPlan
    return FdlpPlan(_cfgs(idx)[0], device=-1, max_frames=MAX_FRAMES)


@functools.lru_cache(maxsize=None)
def _dispatch(idx):
    return _host_plan(idx).autocorr_dispatch()


def _row_paths(idx):
    """The distinct paths the row can launch: 'structured' and 'structured_mfma' where it has them, else 'direct'."""
    d = _dispatch(idx)
    paths = []
    for req in ("structured", "structured_mfma"):
        if req in d and d[req]["path"] not in paths:
            paths.append(d[req]["path"])
    return paths or ["direct"]


# ---- CPU: the table against the dispatch -----------------------------------------------------------------
@pytest.mark.parametrize("idx", range(NROWS), ids=ROW_IDS)
def test_rows_reach_their_instantiation(idx):
    row, d = DISPATCH_ROWS[idx], _dispatch(idx)
    auto = d["auto"]
    print(ROW_IDS[idx], auto)
    for k, v in row[4].items():
        assert auto[k] == v, (ROW_IDS[idx], k, auto)
    plan = _host_plan(idx)
    assert plan.N == int(round(16000 * row[2])) and plan.N <= 8000 and plan.B <= 24
    assert auto["tiles"] == ((plan.nlags + 14) >> 4) + 1 == d["direct"]["tiles"]
    assert d["direct"]["path"] == "direct" and d["direct"]["lanes_lags"] == 0
    if auto["path"] == "direct":
        assert sorted(d) == ["auto", "direct"]
        return
    assert d["structured_mfma"]["path"] == "structured_mfma" and d["structured_mfma"]["lanes_lags"] == 0
    assert d["structured"] == auto
    C, H, ev = plan.flat_events()
    if auto["path"] == "structured":
        assert (C, H) == (auto["chains"], auto["parts"]) and auto["fast22_skirt"]
        assert 0 <= auto["fast_bands"] <= plan.B and (auto["wrap_shared"] or auto["fast_bands"] == 0)
    else:
        assert (C, H) == (0, 0) and not auto["wrap_shared"] and auto["fast_bands"] == 0


def test_table_covers_dispatch_space():
    autos = [_dispatch(i)["auto"] for i in range(NROWS)]
    vs = [a for a in autos if a["path"] == "structured"]
    # every <A, C> of the two switches, with every chain slot in use and two position parts
    full = {(a["lanes_lags"], a["chain_slots"]) for a in vs if a["chains"] == a["chain_slots"] and a["parts"] == 2}
    assert full == {(A, C) for A in ALL_A for C in ALL_C}, full
    assert {(a["lanes_lags"], a["chain_slots"]) for a in vs} == full   # and no instantiation beyond those
    # both plain-run forms at every A that has both
    for A in ALL_A:
        assert {a["fast22_flat"] for a in vs if a["lanes_lags"] == A} == FAST22_FORMS[A], A
    forms = {(a["lanes_lags"], a["chain_slots"]): a["fast22_flat"] for a in vs}
    assert not forms[(8, 4)] and forms[(8, 5)] and forms[(8, 6)] and forms[(8, 8)]
    assert forms[(10, 4)] and forms[(10, 5)] and not forms[(10, 6)] and not forms[(10, 8)]
    # one and two position parts at every C; an idle chain slot; fewer chains than the smallest C
    for C in ALL_C:
        assert {a["parts"] for a in vs if a["chain_slots"] == C} == {1, 2}, C
    assert any(a["chains"] == 7 and a["chain_slots"] == 8 for a in vs)
    assert any(a["chains"] == 1 and a["chain_slots"] == 4 for a in vs)
    # the threshold between one and two parts (flat_parts: a flat range of 2048 positions) lies between the rows
    spans = {}
    for i in VS_ROWS:
        m1, m2 = _host_plan(i).regions()
        spans.setdefault(autos[i]["parts"], []).append(int(m2.max() - m1.min()))
    assert max(spans[1]) < 2048 <= min(spans[2]), spans
    # ac_wrap_kernel on and off; bands on both sides of ac_band_kernel's `fast` staging, also inside one row
    assert {a["wrap_shared"] for a in vs} == {False, True}
    assert any(a["fast_bands"] == 0 for a in vs)
    assert any(0 < _dispatch(i)["auto"]["fast_bands"] < _host_plan(i).B for i in VS_ROWS)
    # the three default paths, and the last order with VALU sweeps next to the first without
    assert {a["path"] for a in autos} == {"direct", "structured", "structured_mfma"}
    by_order = {DISPATCH_ROWS[i][3]: autos[i]["path"] for i in range(NROWS) if DISPATCH_ROWS[i][:3] == (C1, 10, 0.5)}
    assert by_order[158] == "structured" and by_order[159] == "structured_mfma"
    # the event path of the flat sweep, per A: two events inside one block of A positions, and events at every
    # residue of S mod A
    for A in ALL_A:
        two, residues = False, set()
        for i in VS_ROWS:
            if autos[i]["lanes_lags"] != A:
                continue
            plan = _host_plan(i)
            m1, m2 = plan.regions()
            S = plan.flat_events()[2][:, 0].astype(np.int64)
            assert sorted(S.tolist()) == sorted(m1.tolist() + m2.tolist())
            two = two or bool((np.unique(S // A, return_counts=True)[1] >= 2).any())
            row_res = set((S % A).tolist())
            if len(row_res) == A:
                residues = row_res
        assert two, A
        assert residues == set(range(A)), (A, residues)   # within one row's sweep


def test_edge_rows_have_their_edges():
    by_id = {ROW_IDS[i][:2]: i for i in range(NROWS)}
    # row 18: one band with m1 = 0, so the lower-skirt sweep's range [N - m1, N) is empty
    plan = _host_plan(by_id["18"])
    m1, m2 = plan.regions()
    info, rec = plan.sweep_schedule(0)
    assert m1.tolist() == [0] and info["nlo"] == info["nhi"] == plan.N and rec[0, 1] == 2
    # row 19: the last band's flat top reaches N, its upper-skirt snapshot is taken before any position
    plan = _host_plan(by_id["19"])
    m1, m2 = plan.regions()
    assert m2[-1] == plan.N and plan.sweep_schedule(1)[0]["nhi"] == plan.N
    # row 20: flat tops of width 0 (restart and emission at one position) and 1
    m1, m2 = _host_plan(by_id["20"]).regions()
    assert sorted(set((m2 - m1).tolist())) == [0, 1] and int(((m2 - m1) == 0).sum()) == 8
    # rows 21 / 22: nlags = 160 and 161
    assert _host_plan(by_id["21"]).nlags == 160 and _host_plan(by_id["22"]).nlags == 161
    # row 16: the plan's minimum frame length
    assert _host_plan(by_id["16"]).N == 1024


def test_host_plan_dispatch_of_the_recipes():
    """The recipes' plan: <10, 5> in two parts, 2x2 plain runs, the shared wrap and 72 of 80 bands staged `fast`
    (ac_band_kernel's comment); the accessor does not change the plan's path."""
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig
    plan = FdlpPlan(FeatureConfig.wsj(), device=-1)
    d = plan.autocorr_dispatch()
    assert d["auto"] == dict(path="structured", tiles=11, lanes_lags=10, chains=5, chain_slots=5, parts=2,
                             fast22_skirt=True, fast22_flat=True, wrap_shared=True, fast_bands=72)
    assert d["structured_mfma"] == dict(path="structured_mfma", tiles=11, lanes_lags=0, chains=0, chain_slots=0,
                                        parts=0, fast22_skirt=False, fast22_flat=False, wrap_shared=False,
                                        fast_bands=0)
    plan.set_autocorr_path("direct")
    assert plan.autocorr_dispatch() == d and plan.autocorr_path == "direct"
    mel = FdlpPlan(FeatureConfig(fbank_type="mel,1", nfilters=10, fduration=0.5, order=20, coeff_num=10,
                                 coeff_range="0,10"), device=-1)
    assert sorted(mel.autocorr_dispatch()) == ["auto", "direct"]


# ---- inputs and the oracle ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _length_for_frames(idx, F):
    """The shortest utterance (in steps of 50 samples) that the plan cuts into F frames."""
    plan = _host_plan(idx)
    for T in range(50, 16000 * 40, 50):
        if plan.geometry(T)[0] == F:
            return T
    raise AssertionError("no utterance length gives %d frames" % F)


def _signal(name, T, F, seed):
    """The inputs of test_vsweep_block_order.py (speech, white) and test_vsweep_fastcorr.py (the other three)."""
    rng = np.random.default_rng(seed)
    if name == "speech":
        t = np.arange(T) / 16000.0
        return (3000 * np.sin(2 * np.pi * 180 * t) * (1 + np.sin(2 * np.pi * 3 * t))
                + 200 * rng.standard_normal(T)).astype(np.int16)
    if name == "white":
        return (rng.standard_normal(T) * 8000).astype(np.int16)
    if name == "impulse":
        x = np.zeros(T, dtype=np.int16)
        x[[int(T * (2 * i + 1) / (2 * F)) for i in range(F)]] = 32767
        return x
    if name == "alternating":
        return (32767 * (1 - 2 * (np.arange(T) % 2))).astype(np.int16)
    assert name == "lsb"
    return rng.integers(-1, 2, size=T).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _oracle(idx):
    return O.FdlpOracle(_cfgs(idx)[1])


def _autocorr(idx, D):
    """The oracle's autocorrelation of the band signals fbank . D (features.py:190-191, :223-226): [F, B, nlags]."""
    orc = _oracle(idx)
    F, B = D.shape[0], orc.cfg.nfilters
    bands = orc.fbank[None, :, :-1] * D[:, None, :]
    return O.autocorr_fft(bands.reshape(F * B, -1), orc.cfg.order + 2).reshape(F, B, -1)


@functools.lru_cache(maxsize=None)
def _case(idx, name, batch):
    """(utterances, lengths, the oracle's dct and r from the PCM), computed once per case and left unchanged."""
    orc = _oracle(idx)
    sigs = []
    for u, F in enumerate(BATCHES[batch]):
        T = _length_for_frames(idx, F)
        sigs.append(_signal(name, T, F, 1000 * (idx + 1) + 10 * F + u))
    D = np.concatenate([O.dct_frames(O.frames(x, orc.cfg, orc.g), orc.g) for x in sigs])
    assert D.shape[0] == sum(BATCHES[batch])
    r = _autocorr(idx, D)
    assert np.abs(r[..., 0]).min() > 0
    r.setflags(write=False)
    return sigs, [x.size for x in sigs], D, r


@pytest.mark.parametrize("idx", range(NROWS), ids=ROW_IDS)
def test_oracle_is_inside_the_bar(idx):
    """The oracle's circular FFT autocorrelation against the same sum in long double over the same band signals."""
    fbank = _oracle(idx).fbank
    for name in INPUTS:
        _, _, D, r = _case(idx, name, "F1")
        bands = (fbank[:, :-1] * D[0][None, :]).astype(np.longdouble)
        ext = np.concatenate([bands, bands[:, :r.shape[-1]]], axis=1)
        N = bands.shape[1]
        ref = np.stack([(bands * ext[:, lag:lag + N]).sum(axis=1) for lag in range(r.shape[-1])], axis=1)
        rel = float((np.abs(r[0] - ref) / np.abs(r[0][:, :1])).max())
        print(ROW_IDS[idx], name, "oracle against long double", rel)
        assert rel <= ORACLE_TOL, (name, rel)


# ---- GPU ---------------------------------------------------------------------------------------------------
AC_KERNELS = {"fdlp::ac_vsweep_kernel<skirts>", "fdlp::ac_vsweep_kernel<flat>", "fdlp::ac_wrap_kernel",
              "fdlp::ac_band_kernel", "fdlp::ac_sweep_kernel", "fdlp::autocorr_kernel"}


def _expected_kernels(disp):
    if disp["path"] == "direct":
        return {"fdlp::autocorr_kernel"}
    if disp["path"] == "structured_mfma":
        return {"fdlp::ac_sweep_kernel", "fdlp::ac_band_kernel"}
    vs = {"fdlp::ac_vsweep_kernel<skirts>", "fdlp::ac_vsweep_kernel<flat>", "fdlp::ac_band_kernel"}
    return vs | ({"fdlp::ac_wrap_kernel"} if disp["wrap_shared"] else set())


def _device_plan(idx):
    from speech_recognition_tools_amd import FdlpPlan
    plan = FdlpPlan(_cfgs(idx)[0], device=0, max_frames=MAX_FRAMES)
    assert plan.autocorr_dispatch() == _dispatch(idx) and plan.autocorr_path == DISPATCH_ROWS[idx][4]["path"]
    return plan


def _run(plan, sigs, lens, nframes):
    import torch

    from speech_recognition_tools_amd import PyRandom
    jit = PyRandom(0).randbits2(nframes - len(lens))
    plan.compute(torch.from_numpy(np.concatenate(sigs)).cuda(), lens, jit)
    torch.cuda.synchronize()
    return plan.debug_fetch(nframes, keys=("dct", "r"))


def measure_row(idx, batches=tuple(BATCHES), inputs=INPUTS):
    """{"cases": {"input/batch/path": [own, e2e]}, "cross": {"input/batch": structured against structured_mfma},
    "kernels": {path: launched autocorrelation kernels}, "launches_ok": bool}, all errors of r[0]."""
    plan = _device_plan(idx)
    paths = _row_paths(idx)
    disp = _dispatch(idx)
    res = dict(cases={}, cross={}, kernels={}, launches_ok=True)
    got = {}
    for path in paths:
        plan.set_autocorr_path(path)
        assert plan.autocorr_path == path
        plan.set_profiling(True, kernels=True)
        ncalls = 0
        for name in inputs:
            for batch in batches:
                sigs, lens, _, r_ref = _case(idx, name, batch)
                nf = r_ref.shape[0]
                d = _run(plan, sigs, lens, nf)
                ncalls += 1
                r = d["r"]
                assert r.shape == r_ref.shape and np.isfinite(r).all()
                r_own = _autocorr(idx, d["dct"])
                own = float((np.abs(r - r_own).max(axis=-1) / np.abs(r_own[..., 0])).max())
                e2e = float((np.abs(r - r_ref).max(axis=-1) / np.abs(r_ref[..., 0])).max())
                res["cases"]["%s/%s/%s" % (name, batch, path)] = [own, e2e]
                got[(name, batch, path)] = r
        times = plan.kernel_times()
        launched = set(times) & AC_KERNELS
        res["kernels"][path] = sorted(launched)
        want = _expected_kernels(disp[path])
        if launched != want or any(times[k][1] != ncalls for k in want):
            res["launches_ok"] = False
        plan.set_profiling(False)
    if len(paths) == 2:
        for name in inputs:
            for batch in batches:
                a, b = got[(name, batch, paths[0])], got[(name, batch, paths[1])]
                scale = np.abs(_case(idx, name, batch)[3][..., :1])
                res["cross"]["%s/%s" % (name, batch)] = float((np.abs(a - b) / scale).max())
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(NROWS), ids=ROW_IDS)
def test_row(idx):
    res = measure_row(idx)
    print("row %s dispatch %s" % (ROW_IDS[idx], json.dumps(_dispatch(idx)["auto"])))
    for case, (own, e2e) in res["cases"].items():
        print("  %-40s own %.3g e2e %.3g" % (case, own, e2e))
    for case, cross in res["cross"].items():
        print("  %-40s cross %.3g" % (case, cross))
    print("  kernels %s" % json.dumps(res["kernels"]))
    assert len(res["cases"]) == len(INPUTS) * len(BATCHES) * len(_row_paths(idx))
    for case, (own, e2e) in res["cases"].items():
        assert own <= TOL, (ROW_IDS[idx], case, "own", own)
        if case.split("/")[0] in E2E_ASSERTED:
            assert e2e <= TOL, (ROW_IDS[idx], case, "e2e", e2e)
    for case, cross in res["cross"].items():
        assert cross <= 2 * TOL, (ROW_IDS[idx], case, "cross", cross)
    # the skirt and flat VALU sweeps were launched on 'structured' of the rows that have them, and nowhere else
    assert res["launches_ok"], (ROW_IDS[idx], res["kernels"])
    has_vs = "fdlp::ac_vsweep_kernel<flat>" in res["kernels"].get("structured", [])
    assert has_vs == (idx in VS_ROWS)


# ---- the range-check build ---------------------------------------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_autocorr_dispatch as T
from speech_recognition_tools_amd.plan import device_checks
assert device_checks(reset=True)[0], "not a checks build"
runs = 0
for idx in range(T.NROWS):
    sigs, lens, _, r = T._case(idx, "white", "F5")
    T._run(T._device_plan(idx), sigs, lens, r.shape[0])
    runs += 1
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": runs}))
"""


@pytest.mark.gpu
def test_rows_under_range_checks():
    """Every row once at F = 5 through the library built with -DFDLP_DEVICE_CHECKS=1 (one child process: the
    library is chosen when it is loaded): ring slots, staged ranges, parked rows, chain and part indices of every
    ac_vsweep_kernel instantiation and ac_band_kernel's straddle windows stay inside their ranges."""
    assert os.path.exists(CHECKS_LIB), "build() compiles libfdlp_checks.so"
    env = dict(os.environ, FDLP_LIB=CHECKS_LIB)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["enabled"] and res["runs"] == NROWS
    assert res["violations"] == 0, res


# ---- the recorded measurements -----------------------------------------------------------------------------
def worst_values(records):
    """{quantity: (value, row, case)} over the recorded rows."""
    worst = {k: (0.0, "", "") for k in MEASURED_WORST}
    for rec in records:
        for case, (own, e2e) in rec["cases"].items():
            key = "e2e" if case.split("/")[0] in E2E_ASSERTED else "e2e_alternating"
            for q, v in (("own", own), (key, e2e)):
                if v > worst[q][0]:
                    worst[q] = (float("%.3g" % v), rec["row"], case)
        for case, v in rec["cross"].items():
            if v > worst["cross"][0]:
                worst["cross"] = (float("%.3g" % v), rec["row"], case)
    return worst


def test_recorded_errors_match_docstring():
    """tests/data/autocorr_dispatch_errors.jsonl holds one record per row with every input, batch and path, every
    asserted value is within its bar, and MEASURED_WORST quotes that file's worst values."""
    assert os.path.exists(ERRORS_FILE)
    recs = [json.loads(l) for l in open(ERRORS_FILE)]
    assert [r["row"] for r in recs] == ROW_IDS
    for idx, rec in enumerate(recs):
        assert sorted(rec["cases"]) == sorted("%s/%s/%s" % (n, b, p) for n in INPUTS for b in BATCHES
                                              for p in _row_paths(idx)), rec["row"]
        assert rec["launches_ok"] and rec["dispatch"] == _dispatch(idx)["auto"]
    worst = worst_values(recs)
    assert worst["own"][0] <= TOL and worst["e2e"][0] <= TOL and worst["cross"][0] <= 2 * TOL, worst
    assert worst == MEASURED_WORST


def record(path=ERRORS_FILE):
    with open(path, "w") as f:
        for idx in range(NROWS):
            res = measure_row(idx)
            f.write(json.dumps(dict(row=ROW_IDS[idx], dispatch=_dispatch(idx)["auto"], **res)) + "\n")
            f.flush()
    print("MEASURED_WORST = %r" % (worst_values([json.loads(l) for l in open(path)]),))


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_autocorr_dispatch.py --record [file]")
    rest = [a for a in sys.argv[1:] if a != "--record"]
    record(rest[0] if rest else ERRORS_FILE)
