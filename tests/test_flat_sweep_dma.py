"""The flat sweep's two staging forms (ac_vsweep_kernel<A, C>, csrc/fdlp_autocorr.hip): D copied into the LDS ring
by LDS-DMA (global_load_lds_dwordx4, the default where the D rows are 16-byte aligned, i.e. N even) against D staged
through registers (FdlpPlan.set_flat_staging("register")).  Staging changes when and how a chunk reaches the ring,
not one operand of one FMA, so the check is equality: r of the two forms agrees bit for bit, and each is within the
project's 1e-12 of r[0] of the oracle's autocorrelation of the device's own dct.

The cases are rows of tests/test_autocorr_dispatch.py's table (its plans, inputs, batches, oracle and stage entry
are imported, the oracle's values shared with that file), picked for what the DMA form can get wrong:

* N = 1024 (row 16): two ring revolutions, so chunks land on slots that were read before (WAR) and the chunk at
  slot 0 fills the mirror behind the ring twice;
* N = 8000 and N = 1600, even and no multiple of the 128-position chunk: the sweep's first chunks reach past N
  (clamped source, zeroed slots) or lie wholly above it (no copy, zeros);
* one-part (rows 14 to 19) and two-part flat sweeps, the second part's first chunks lying inside the row;
* row 18: a flat sweep of 51 positions, shorter than one chunk;
* F = 1, F = 5 and 2 + 4 frames: one, three and two frame rows past the batch's end in the last wave;
* every <A, C> the launcher has, <10, 4> and <10, 5> (the recipes') among them, with every chain slot in use;
* the five inputs of the dispatch file (speech-like, white, impulse, alternating, 1-LSB noise).

An odd N (1215 = 3^5 5) has rows that are not 16-byte aligned: the plan reports the register form, 'auto' and
'register' are then the same kernel, and it meets the oracle like the others.  test_cases_under_range_checks runs
every case through libfdlp_checks.so, which checks each copy's source range against its D row and its
destination against the ring and the mirror: zero violations.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_autocorr_dispatch as T
from conftest import ROOT
from oracle import fdlp_oracle as O

CASE_ROWS = list(T.VS_ROWS)   # every row that launches the VALU sweeps
ODD_N = 1215
ODD_ROW = (T.C8, 12, (ODD_N + 0.5) / 16000.0, 150)


def test_cases_reach_their_hazards():
    """CPU: the table's rows have the shapes the docstring names, and every one of them takes the DMA form."""
    seen, parts, short = set(), set(), False
    for idx in CASE_ROWS:
        plan, auto = T._host_plan(idx), T._dispatch(idx)["auto"]
        assert plan.N % 2 == 0 and plan.flat_staging == "dma", T.ROW_IDS[idx]
        plan.set_flat_staging("register")
        assert plan.flat_staging == "register"
        plan.set_flat_staging("auto")
        assert plan.flat_staging == "dma"
        seen.add((auto["lanes_lags"], auto["chain_slots"]))
        parts.add(auto["parts"])
        for h in range(auto["parts"]):
            info = plan.sweep_schedule(2, h)[0]
            assert info["chunk"] == 128
            short = short or 0 < info["nhi"] - info["nlo"] < 128
    assert seen == {(A, C) for A in T.ALL_A for C in T.ALL_C} and parts == {1, 2} and short
    Ns = {T._host_plan(idx).N for idx in CASE_ROWS}
    assert 1024 in Ns and any(N % 128 for N in Ns)
    # the fallbacks have no VALU sweeps and so no staging form
    for idx in set(range(T.NROWS)) - set(CASE_ROWS):
        assert T._host_plan(idx).flat_staging is None


def _odd_cfgs():
    from speech_recognition_tools_amd import FeatureConfig
    fb, nf, fd, order = ODD_ROW
    kw = dict(fbank_type=fb, nfilters=nf, fduration=fd, order=order, coeff_num=T.COEFF_NUM,
              coeff_range="0,%d" % T.COEFF_NUM)
    return FeatureConfig(**kw), O.FdlpConfig(**kw)


def test_odd_frame_length_keeps_the_register_form():
    """CPU: rows of an odd N are not 16-byte aligned, so the plan stays on the register form whatever is asked."""
    from speech_recognition_tools_amd import FdlpPlan
    plan = FdlpPlan(_odd_cfgs()[0], device=-1, max_frames=T.MAX_FRAMES)
    auto = plan.autocorr_dispatch()["auto"]
    assert plan.N == ODD_N and auto["path"] == "structured" and (auto["lanes_lags"], auto["chain_slots"]) == (10, 5)
    for req in ("auto", "register", "auto"):
        plan.set_flat_staging(req)
        assert plan.flat_staging == "register"


# ---- GPU ---------------------------------------------------------------------------------------------------
def _both_forms(plan, sigs, lens, nframes):
    """(r by the default staging, r by the forced register form, the device's dct)."""
    plan.set_flat_staging("auto")
    d = T._run(plan, sigs, lens, nframes)
    plan.set_flat_staging("register")
    assert plan.flat_staging == "register"
    e = T._run(plan, sigs, lens, nframes)
    plan.set_flat_staging("auto")
    assert np.array_equal(d["dct"], e["dct"])
    return d["r"], e["r"], d["dct"]


@pytest.mark.gpu
@pytest.mark.parametrize("idx", CASE_ROWS, ids=[T.ROW_IDS[i] for i in CASE_ROWS])
def test_dma_equals_register_form(idx):
    plan = T._device_plan(idx)
    assert plan.autocorr_path == "structured" and plan.flat_staging == "dma"
    plan.set_profiling(True, kernels=True)
    ncalls = 0
    for name in T.INPUTS:
        for batch in T.BATCHES:
            sigs, lens, _, r_ref = T._case(idx, name, batch)
            r_dma, r_reg, dct = _both_forms(plan, sigs, lens, r_ref.shape[0])
            ncalls += 2
            assert r_dma.shape == r_ref.shape and np.isfinite(r_dma).all()
            r_own = T._autocorr(idx, dct)
            errs = [float((np.abs(r - r_own).max(axis=-1) / np.abs(r_own[..., 0])).max()) for r in (r_dma, r_reg)]
            ndiff = int((r_dma.view(np.uint64) != r_reg.view(np.uint64)).sum())
            print("%s %-12s %-5s own: dma %.3g register %.3g, words that differ %d"
                  % (T.ROW_IDS[idx], name, batch, errs[0], errs[1], ndiff))
            assert ndiff == 0, (T.ROW_IDS[idx], name, batch, ndiff)
            assert max(errs) <= T.TOL, (T.ROW_IDS[idx], name, batch, errs)
    times = plan.kernel_times()
    assert times["fdlp::ac_vsweep_kernel<flat>"][1] == ncalls   # both forms are the flat launch
    plan.set_profiling(False)


@functools.lru_cache(maxsize=None)
def _odd_case(name, batch):
    fcfg, ocfg = _odd_cfgs()
    from speech_recognition_tools_amd import FdlpPlan
    host = FdlpPlan(fcfg, device=-1, max_frames=T.MAX_FRAMES)
    sigs = []
    for u, F in enumerate(T.BATCHES[batch]):
        Tn = next(t for t in range(50, 16000 * 40, 50) if host.geometry(t)[0] == F)
        sigs.append(T._signal(name, Tn, F, 77000 + 10 * F + u))
    return sigs, [x.size for x in sigs], sum(T.BATCHES[batch])


@pytest.mark.gpu
def test_odd_frame_length_on_the_device():
    from speech_recognition_tools_amd import FdlpPlan
    fcfg, ocfg = _odd_cfgs()
    orc = O.FdlpOracle(ocfg)
    plan = FdlpPlan(fcfg, device=0, max_frames=T.MAX_FRAMES)
    assert plan.N == ODD_N and plan.autocorr_path == "structured" and plan.flat_staging == "register"
    for name in T.INPUTS:
        for batch in T.BATCHES:
            sigs, lens, nf = _odd_case(name, batch)
            r_auto, r_reg, dct = _both_forms(plan, sigs, lens, nf)
            bands = orc.fbank[None, :, :-1] * dct[:, None, :]
            r_own = O.autocorr_fft(bands.reshape(nf * orc.cfg.nfilters, -1), orc.cfg.order + 2).reshape(r_auto.shape)
            err = float((np.abs(r_auto - r_own).max(axis=-1) / np.abs(r_own[..., 0])).max())
            print("N %d %-12s %-5s own %.3g" % (ODD_N, name, batch, err))
            assert np.array_equal(r_auto.view(np.uint64), r_reg.view(np.uint64))
            assert err <= T.TOL, (name, batch, err)


# ---- the range-check build ---------------------------------------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_autocorr_dispatch as T
import test_flat_sweep_dma as D
from speech_recognition_tools_amd.plan import device_checks
assert device_checks(reset=True)[0], "not a checks build"
runs = 0
for idx in D.CASE_ROWS:
    plan = T._device_plan(idx)
    assert plan.flat_staging == "dma"
    for name in T.INPUTS:
        for batch in T.BATCHES:
            sigs, lens, _, r = T._case(idx, name, batch)
            T._run(plan, sigs, lens, r.shape[0])
            runs += 1
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": runs}))
"""


@pytest.mark.gpu
def test_cases_under_range_checks():
    """Every case above, in the DMA form, through the library built with -DFDLP_DEVICE_CHECKS=1 (one child
    process: the library is chosen when it is loaded): each copy's source inside its D row, its destination
    inside the ring, the edge zeros and the mirror copy inside the row."""
    assert os.path.exists(T.CHECKS_LIB), "build() compiles libfdlp_checks.so"
    env = dict(os.environ, FDLP_LIB=T.CHECKS_LIB)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["enabled"] and res["runs"] == len(CASE_ROWS) * len(T.INPUTS) * len(T.BATCHES)
    assert res["violations"] == 0, res
