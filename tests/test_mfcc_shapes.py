"""mfcc_kernel<RT> (fdlp_mfcc.hip) at every tile shape its plan can pick, held to a derived error bound.

The kernel's shape follows from nfft, fduration and nfilters: one or two 16-frame row tiles (whichever fits the
LDS), nbpad / 16 column tiles handed to four waves kMfccNT at a time (a second and third trip of the wave loop
past 20 and 40 tiles, with the tiles past the last one aliased), K = min(L, n) frame samples padded to a multiple
of 4, and the log-mel tile written over the frame tile with stride max(Kpad, nfilters) + 2.  SHAPE_ROWS
(tests/golden/make_golden_mfcc.py) has one small case per reachable shape; test_table_covers_shape_space holds
the table to the plan, so a changed constant fails here until the table follows.

The bar is oracle.mfcc_oracle.cep_bound: the error a float64 evaluation of the chain can make, derived from the
arithmetic (dot products in any order, hypot, the folded filterbank, log10, the DCT-II) and evaluated from a
longdouble run of the same chain.  Two conditions are checked on the CPU for every row and fixture before a GPU
is involved: (1) the real reference's output (the float64 restatement where a row has no fixture) lies within
the bound at every element; (2) no element of the bound exceeds 1e-7 and e_lin <= 2^-20 lin for every filter
with taps, so an ill-conditioned input cannot hide a failure.  The 'empty' row (filters without taps: log10(0))
has no finite values; only its non-finite mask is compared.

Measured.  Bound maxima per case: 7e-12 .. 2.8e-9, 1.7e-8 (n636) and 3.1e-8 (k800) with their 5-sample
utterance, 1.1e-12 at K = 17.  Worst |err| / bound on the CPU, reference fixtures and the scipy restatement:
1.3e-4 .. 8.7e-4, 4.3e-3 at K = 32 (widemel) and 2.4e-2 at K = 17 (tiny).  On the MI355X, out64 against the
longdouble oracle: 3.4e-4 .. 1.3e-3, 9.5e-3 (widemel), 1.8e-2 (tiny); against the reference fixtures 3.6e-4 ..
1.5e-3, 3.1e-2 (tiny).  The n638 row's one-frame utterance has 7 samples, not 5: see ONE_FRAME_OF.
"""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from test_mfcc import MFCC_SETS, _cfg, _evaluate, _mfcc_gpu, _ratio, _reference_inputs

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_mfcc as G  # noqa: E402  (the row table and the input recipes; nothing of the reference is run)

ROW_IDS = [r[0] for r in G.SHAPE_ROWS]
ROW = {rid: i for i, rid in enumerate(ROW_IDS)}
CASES = ROW_IDS + ["ctx7"] + MFCC_SETS
BOUND_CAP = 1e-7
CHECK_ROWS = ["n1214", "n1280", "n2048", "tiny", "widemel"]
CHECKS_LIB = os.path.join(ROOT, "speech_recognition_tools_amd", "lib", "libfdlp_checks.so")
WAVES = 4
ld = np.longdouble


@functools.lru_cache(maxsize=None)
def _case(name):
    """dict(meta, sig, ref or None, x (the float64 signals entering getFrames), and per utterance the longdouble
    evaluation's feats, the bound, e_lin / lin and the float64 restatement); computed once, never modified."""
    if name in ROW:
        _, over, _, fixture = G.SHAPE_ROWS[ROW[name]]
        sig = G.shape_row_signals(ROW[name])
        meta = dict(opts=G.shape_row_opts(over), utts=list(sig), extra={})
        fx = "mfcc_shape_" + name if fixture else None
    elif name == "ctx7":
        sig = G.shape_ctx_signals()
        meta = dict(opts=G.shape_row_opts(G.SHAPE_CTX), utts=list(sig), extra={})
        fx = "mfcc_shape_ctx7"
    else:
        sig, fx = None, name
    ref, z = None, None
    if fx:
        fmeta, fsig, ref, z = load_golden(fx)
        if sig is None:
            meta, sig = fmeta, fsig
        assert fmeta["opts"] == meta["opts"] and fmeta["utts"] == meta["utts"], fx
        for u in meta["utts"]:  # the fixture was made from the recipe's signals
            assert fsig[u].dtype == np.int16 and np.array_equal(fsig[u], sig[u]), (fx, u)
    xs = _reference_inputs(meta, sig, z)
    return dict(name=name, meta=meta, sig=sig, ref=ref, z=z, x=xs, **_evaluate(meta["opts"], xs))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=str(what))


def _kernel_constants():
    src = open(os.path.join(ROOT, "speech_recognition_tools_amd", "csrc", "fdlp_mfcc.hip")).read()
    nt = int(re.search(r"constexpr int kMfccNT = (\d+);", src).group(1))
    lds = re.search(r"constexpr int kMfccLdsMax = (\d+) \* 1024;", src).group(1)
    return nt, int(lds) * 1024


def _column_passes(nbpad, nt, wave=0):
    """trips of `for (j0 = 0; wave + 4 * j0 < nct; j0 += kMfccNT)`"""
    nct, j0, trips = nbpad // 16, 0, 0
    while wave + WAVES * j0 < nct:
        trips += 1
        j0 += nt
    return trips


def _lds_bytes(rt, Kpad, nbpad, nfilters):
    sa = max(Kpad, nfilters) + 2
    while sa % 32 != 2:
        sa += 1
    return 8 * 16 * rt * (sa + nbpad + 1)


def _host_plan(opts):
    from speech_recognition_tools_amd.mfcc import MfccPlan
    return MfccPlan(_cfg(dict(opts=opts)), device=-1)


# ---------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------
def test_table_covers_shape_space():
    nt, lds_max = _kernel_constants()
    seen = {}
    for rid, over, M, _ in G.SHAPE_ROWS:
        o = G.shape_row_opts(over)
        t = _host_plan(o).tables()
        L, hop = int(16000 * o["fduration"]), int(16000 / o["frate"])
        assert t["tile"] == M, (rid, t["tile"])
        assert (t["n"], t["nb"], t["K"]) == (o["nfft"] // 2 + 1, (o["nfft"] // 2 + 1) // 2 + 1, min(L, t["n"])), rid
        rt = t["tile"] // 16
        assert _lds_bytes(rt, t["Kpad"], t["nbpad"], o["nfilters"]) <= lds_max, rid
        assert rt == 2 or _lds_bytes(2, t["Kpad"], t["nbpad"], o["nfilters"]) > lds_max, rid
        seen[rid] = dict(t, L=L, hop=hop, nct=t["nbpad"] // 16, passes=_column_passes(t["nbpad"], nt),
                         lds=_lds_bytes(rt, t["Kpad"], t["nbpad"], o["nfilters"]))
    rows = seen.values()
    assert {r["tile"] for r in rows} == {16, 32}
    assert {r["passes"] for r in rows} == {1, 2, 3}
    assert any(r["nct"] < WAVES for r in rows)                                # waves without a column tile
    assert any(r["K"] % 4 for r in rows)                                      # a zero-padded k-step
    assert any(r["nfilters"] > r["Kpad"] for r in rows)                       # log-mel tile wider than the frames
    assert {r["L"] % 2 for r in rows} == {0, 1} and {r["n"] % 2 for r in rows} == {0, 1}
    assert any(r["L"] < r["n"] for r in rows) and any(r["L"] == r["n"] for r in rows)
    assert any(r["L"] > r["n"] for r in rows)
    assert any(r["L"] == r["n"] + 1 for r in rows) and any(r["L"] == r["n"] - 1 for r in rows)
    assert any(r["hop"] > r["L"] for r in rows) and any(r["hop"] < r["L"] for r in rows)
    assert any(r["ncep"] < 13 for r in rows) and any(r["nfilters"] > 13 for r in rows)
    # both thresholds are bracketed by rows one step apart
    a, b, c = seen["n1212"], seen["n1214"], seen["n1278"]
    assert (a["tile"], b["tile"]) == (32, 16) and (a["K"], b["K"]) == (320, 320) and b["n"] - a["n"] == 1
    assert (a["lds"], a["nct"]) == (160512, 19)
    assert (b["nct"], b["passes"]) == (WAVES * nt, 1) and (c["nct"], c["passes"]) == (WAVES * nt + 1, 2)
    for rid in ("n1278", "n1280", "n1282"):                                   # tile 20 on wave 0 alone
        assert seen[rid]["nct"] == 21
        assert [_column_passes(seen[rid]["nbpad"], nt, w) for w in range(WAVES)] == [2, 1, 1, 1]
    assert (seen["n2048"]["nct"], seen["n2048"]["passes"], seen["n2048"]["tile"]) == (33, 2, 16)
    assert (seen["n3000"]["nct"], seen["n3000"]["passes"], seen["n3000"]["lds"]) == (47, 3, 137600)
    assert (seen["k800"]["K"], seen["k800"]["nct"], seen["k800"]["lds"]) == (800, 26, 156032)
    assert (seen["tiny"]["n"], seen["tiny"]["K"], seen["tiny"]["Kpad"], seen["tiny"]["nct"]) == (17, 17, 20, 1)
    assert seen["tiny"]["L"] < seen["tiny"]["hop"] and seen["tiny"]["ncep"] == 5
    assert (seen["widemel"]["K"], seen["widemel"]["nfilters"]) == (32, 40)
    odd = seen["oddL"]
    assert (odd["L"], odd["Kpad"], odd["lds"], odd["tile"]) == (321, 324, 160512, 32)
    assert (seen["hop533"]["hop"], seen["hop128"]["hop"]) == (533, 128)
    fold = seen["empty"]["fold"]
    assert int((~fold.any(axis=1)).sum()) == 14 and fold.shape[0] == 40
    assert all(seen[r]["fold"].any(axis=1).all() for r in seen if r != "empty")


@pytest.mark.parametrize("rid", ROW_IDS)
def test_row_inputs_fill_the_tiles(rid):
    c = _case(rid)
    plan = _host_plan(c["meta"]["opts"])
    M = plan.tables()["tile"]
    lens = [c["sig"][u].size for u in c["meta"]["utts"]]
    frames = [plan.frames(T) for T in lens]
    assert frames == [1, M - 1, M + 1, 2] and sum(frames) == 2 * M + 3
    assert lens[0] == G.ONE_FRAME_OF.get(rid, G.ONE_FRAME) and G.ONE_FRAME == 5 and G.ONE_FRAME_OF == {"n638": 7}
    assert lens[0] < int(16000 * c["meta"]["opts"]["fduration"]) // 2 - 1 or rid in ("tiny", "widemel")
    assert all(x.dtype == np.int16 for x in c["sig"].values())


@pytest.mark.parametrize("name", CASES)
def test_oracle_within_bound_and_bound_conditions(name):
    c = _case(name)
    worst = dict(ref=0.0, f64=0.0, bound=0.0, rel_lin=0.0)
    for u in c["meta"]["utts"]:
        exact, bound, f64 = c["exact"][u], c["bound"][u], c["f64"][u]
        ref = c["ref"][u] if c["ref"] is not None else None
        if name == "empty":  # log10(0): nothing finite to bound
            assert not np.isfinite(f64).any() and not np.isfinite(exact).any()
            assert ref is not None and np.array_equal(np.isfinite(ref), np.isfinite(f64))
            continue
        # the oracle against the fixture: the float64 restatement as before, the longdouble one within the bound
        if ref is not None:
            assert np.isfinite(ref).all()
            np.testing.assert_allclose(f64, ref, rtol=0, atol=1e-10)
            worst["ref"] = max(worst["ref"], _ratio(ref, exact, bound, (name, u, "reference")))  # condition 1
        worst["f64"] = max(worst["f64"], _ratio(f64, exact, bound, (name, u, "restatement")))    # condition 1
        # condition 2
        worst["bound"] = max(worst["bound"], float(bound.max()))
        worst["rel_lin"] = max(worst["rel_lin"], float(c["rel_lin"][u].max()))
        assert (bound <= BOUND_CAP).all(), (name, u, float(bound.max()))
        assert (c["rel_lin"][u] <= 2.0 ** -20).all(), (name, u, float(c["rel_lin"][u].max()))
    print("%s: |err|/bound reference %.3g restatement %.3g; max bound %.3g; max e_lin/lin %.3g"
          % (name, worst["ref"], worst["f64"], worst["bound"], worst["rel_lin"]))


# ---------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------
def _device_plan(opts):
    from speech_recognition_tools_amd.mfcc import MfccPlan
    return MfccPlan(_cfg(dict(opts=opts)), device=0, max_frames=256)


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ROW_IDS)
def test_gpu_shape_row(rid):
    c = _case(rid)
    meta, sig, utts = c["meta"], c["sig"], c["meta"]["utts"]
    plan = _device_plan(meta["opts"])
    whole = _mfcc_gpu(meta, sig, None, plan=plan)
    if rid == "empty":
        for u in utts:
            assert whole[u][0].shape == c["ref"][u].shape
            np.testing.assert_array_equal(np.isfinite(whole[u][0]), np.isfinite(c["ref"][u]))
        return
    worst, worst_ref = 0.0, 0.0
    for u in utts:
        f64, f32 = whole[u]
        assert f64.shape == f32.shape == (plan.frames(sig[u].size), 13 if rid != "tiny" else 5), u
        worst = max(worst, _ratio(f64, c["exact"][u], c["bound"][u], (rid, u, "longdouble oracle")))
        if c["ref"] is not None:
            worst_ref = max(worst_ref, _ratio(f64, c["ref"][u].astype(ld), c["bound"][u], (rid, u, "fixture")))
        _assert_same_bits(f32, (np.rint(f64 * 1e3) / 1e3).astype(np.float32), (rid, u, "'%.3f' rounding"))
    print("%s: worst |out64 - oracle| / bound = %.3g, |out64 - reference| / bound = %.3g, max bound %.3g"
          % (rid, worst, worst_ref, max(float(c["bound"][u].max()) for u in utts)))
    for u in utts:
        alone = _mfcc_gpu(meta, sig, None, utts=[u], plan=plan)[u]
        _assert_same_bits(alone[0], whole[u][0], (rid, u, "alone"))
        _assert_same_bits(alone[1], whole[u][1], (rid, u, "alone, float32"))
    for other, what in ((_mfcc_gpu(meta, sig, None, utts=utts[::-1], plan=plan), "reversed"),
                        (_mfcc_gpu(meta, sig, None, plan=plan), "second compute")):
        for u in utts:
            _assert_same_bits(other[u][0], whole[u][0], (rid, u, what))
            _assert_same_bits(other[u][1], whole[u][1], (rid, u, what + ", float32"))


@pytest.mark.gpu
def test_gpu_shape_context():
    """--nfft 2048 --context 7 (mfcc_kernel<1> into the cepstrum scratch, two column passes, then the splice)"""
    c = _case("ctx7")
    meta, sig, utts = c["meta"], c["sig"], c["meta"]["utts"]
    C = meta["opts"]["context"]
    both = _mfcc_gpu(meta, sig, None)
    plain = _mfcc_gpu(dict(meta, opts=dict(meta["opts"], context=None)), sig, None)
    zero_ctx = _mfcc_gpu(dict(meta, opts=dict(meta["opts"], context=0)), sig, None)
    worst = 0.0
    for u in utts:
        f64 = both[u][0]
        F = f64.shape[0]
        assert f64.shape == c["ref"][u].shape == (F, 13 * (2 * C + 1)), u
        assert not _bits(f64[max(F - C, 0):]).any(), u                       # rows F-C .. F-1, all when F <= C: +0.0
        worst = max(worst, _ratio(f64, c["exact"][u], c["bound"][u], (u, "longdouble oracle")))
        worst = max(worst, _ratio(f64, c["ref"][u].astype(ld), c["bound"][u], (u, "fixture")))
        if F > C:
            # the last non-zero row: frames F-2C-1 .. F-1 of this utterance (zeros before frame 0), not the neighbour's
            want = np.zeros(13 * (2 * C + 1))
            lo = F - 2 * C - 1
            want[13 * max(-lo, 0):] = plain[u][0][max(lo, 0):F].reshape(-1)
            _assert_same_bits(f64[F - C - 1], want, (u, "last non-zero row"))
        _assert_same_bits(zero_ctx[u][0], plain[u][0], (u, "context 0 is context None"))
        _assert_same_bits(zero_ctx[u][1], plain[u][1], (u, "context 0 is context None, float32"))
    shapes = {u: both[u][0].shape[0] for u in utts}
    assert shapes == dict(x8=8, x5=5, x20=20)
    assert both["x8"][0][0].any() and not both["x8"][0][1:].any() and not both["x5"][0].any()
    print("ctx7: worst |out64 - oracle or reference| / bound = %.3g" % worst)


CHECKS_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import test_mfcc_shapes as TS_
from test_mfcc import _mfcc_gpu
from speech_recognition_tools_amd.plan import device_checks
assert device_checks(reset=True)[0], "not a checks build"
runs = 0
for rid in TS_.CHECK_ROWS:
    i = TS_.ROW[rid]
    sig = TS_.G.shape_row_signals(i)
    meta = dict(opts=TS_.G.shape_row_opts(TS_.G.SHAPE_ROWS[i][1]), utts=list(sig))
    res = _mfcc_gpu(meta, sig, None)
    assert all(np.isfinite(res[u][0]).all() for u in sig), rid
    runs += 1
sig = TS_.G.shape_ctx_signals()
res = _mfcc_gpu(dict(opts=TS_.G.shape_row_opts(TS_.G.SHAPE_CTX), utts=list(sig)), sig, None)
runs += 1
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": runs}))
"""


@pytest.mark.gpu
def test_gpu_device_range_checks_silent():
    """the FDLP_DEVICE_CHECKS build of mfcc_kernel<1>, mfcc_kernel<2> and mfcc_splice_kernel: frame, sample, LDS,
    twiddle, filter-range and output indices stay in range"""
    assert os.path.exists(CHECKS_LIB), "build() compiles libfdlp_checks.so"
    r = subprocess.run([sys.executable, "-c", CHECKS_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=dict(os.environ, FDLP_LIB=CHECKS_LIB), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["enabled"] and res["runs"] == len(CHECK_ROWS) + 1
    assert res["violations"] == 0, res


@pytest.mark.gpu
def test_gpu_cli_nfft2048_batch_frames(tmp_path):
    """compute-mfcc-feats --nfft 2048 twice, side by side: the default --batch_frames, and 7 -- below one
    utterance's frame count (the plan is re-created) and no multiple of the tile"""
    from scipy.io import wavfile
    from speech_recognition_tools_amd.featgen.features import read_ark
    c = _case("n2048")
    utts = c["meta"]["utts"]
    scp = tmp_path / "wav.scp"
    with open(scp, "w") as f:
        for u in utts:
            p = tmp_path / (u + ".wav")
            wavfile.write(str(p), 16000, c["sig"][u])
            f.write("%s %s\n" % (u, p))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = [str(tmp_path / "default"), str(tmp_path / "bf7")]
    cmd = [os.path.join(ROOT, "bin", "compute-mfcc-feats"), str(scp)]
    ps = [subprocess.Popen(cmd + [out, "--nfft=2048", "--kaldi_cmd=copy-feats"] + extra, cwd=str(tmp_path), env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
          for out, extra in zip(outs, ([], ["--batch_frames=7"]))]
    logs = []
    for p in ps:
        try:
            so, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            so, _ = p.communicate()
        logs.append(so.decode("utf-8", "replace"))
    for p, log in zip(ps, logs):
        assert p.returncode == 0, log[-3000:]
    assert max(c["ref"][u].shape[0] for u in utts) > 7
    arks = [open(out + ".ark", "rb").read() for out in outs]
    assert arks[0] == arks[1]
    for out in outs:
        ark = read_ark(out + ".ark")
        assert list(ark) == utts
        for u in utts:
            assert ark[u].shape == c["ref"][u].shape
            assert np.abs(ark[u] - c["ref"][u]).max() <= 1.001e-3, u
    assert not any(f.endswith(".tmp") for f in os.listdir(str(tmp_path)))
