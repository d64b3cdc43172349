"""The OLA + log output stage (ola_log_tiled_kernel, csrc/fdlp_misc.hip) against numpy on the oracle's ola_plan,
through the stage entry point FdlpPlan.ola_rows (fdlp_ola_rows), which fills the frame / utterance tables with the
code fdlp_compute fills them with and launches the kernel on envelopes the test chooses.

The kernel sums a tile of 32 output rows either in registers (at most 3 frames on the tile and at most 80 bands)
or through an LDS loop, chosen per tile; its dynamic LDS grows with the band count (the large-LDS attribute from
247 bands, refused on the host from 631).  CASES below holds the geometries and lengths that reach each branch:

* test_table_reaches_every_path (CPU): FdlpPlan.ola_info() of host-only plans and O.ola_plan classify every
  (case, B, utterance, tile): register path, LDS loop because of the frames, LDS loop because of the bands, no
  frame on the tile, one-row tile, tile with uncovered rows; no class is empty, one utterance mixes register and
  LDS-loop tiles, and BIG_B / REFUSED_B bracket both LDS thresholds as ola_info() reports them.
* test_reference_* (CPU): O.ola_features is FdlpOracle.utterance's last lines bit for bit, and no row of any case
  is covered by three frames (ola_hop >= kkb2 and frame 0's kk = 2 kkb2 are what plan creation / ola_plan insist
  on), so every fp64 sum has at most two terms, does not depend on its order, and equals numpy's exactly.
* test_rows_against_reference (GPU): every case at B in {1, 7, 80, 81} (+ 246, 247, 630 for three cases), all
  utterances in one launch placed in reverse order with gaps of 1 and 33 rows into sentinel-filled buffers, random
  envelopes exp(3 N(0, 1)) and a set with planted NaN, +inf, 0.0, -0.0, a negative value, 5e-324, 1e-14, the double
  below it and 1e300, at ark_decimals -1, 0, 3, 4: fp64 within 1 ulp of numpy's log (the bar test_device_log.py
  holds ola_log to) with NaN and +inf in numpy's cells, float32 rows and codes the exact functions of the device's
  fp64 value, the flag set exactly when a value has no code, codes alone equal to codes with the other outputs,
  and the sentinel in every row outside an utterance.
* test_an_utterance_does_not_depend_on_its_batch, test_refusals, test_entry_point_is_the_production_path,
  test_rows_under_range_checks (GPU): see each.

The 'tworow' geometry (fduration 0.02) has N = 320 samples at 16 kHz, below the 1024 plan creation accepts, so
it runs at srate 64000 with four times the samples: kk / kkb2 / ola_hop, F and L are those of the 16 kHz lengths
(asserted in test_table_reaches_every_path).

Measured on the MI355X (worst fp64 distance to numpy's log in ulps over all B, decimals and both envelope sets;
every case: NaN / +inf cells identical, float32 rows and codes exact): recipe 1.0, half 1.0, ov50 1.0, short 1.0,
short50 1.0, tworow 1.0, noov 1.0, oddkk 1.0, fr160 1.0 -- one ulp is ola_log's own worst case (fewer than 1 % of
its values are not correctly rounded); 0.0 at recipe / short / short50 / oddkk / fr160 B = 1 and tworow / oddkk
B = 7, where the few hundred values all round correctly.  The LDS thresholds ran at B = 246, 247 and 630 as ola_info()
gives them, 631 is refused; plan creation accepts all of them.  No defect was found.

Hand mutations of ola_log_tiled_kernel (scratch builds): `lo - kf <= kOlaFr` fails test_rows_against_reference at
ov50 / short50 B 1, 7, 80 and test_entry_point_is_the_production_path[ov50-B7], no older test; the register path's
column without fd.src fails test_rows_against_reference at every B <= 80 of eight cases, the production-path test at
B 7, and the older golden / CLI parity tests; `B <= 8 * kOlaJ + 8` fails test_rows_against_reference at B 81 of every
case and the production-path test at B 81, no older test.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, oracle_cfg
from oracle import fdlp_oracle as O

CHECKS_LIB = os.path.join(ROOT, "speech_recognition_tools_amd", "lib", "libfdlp_checks.so")
MAX_FRAMES = 64
SENT64, SENT32, SENTQ = -12345.678, np.float32(-4321.5), 21930
DECIMALS = (-1, 0, 3, 4)

# name: fduration, frate, overlap_fraction, (kk, kkb2, ola_hop), accepted lengths and refused lengths in samples
# at 16 kHz (srate: see the docstring)
CASES = {
    "recipe": dict(fd=1.5, fr=100, ov=0.25, geo=(150, 75, 112), T=(100, 5121, 16000, 40000)),
    "half": dict(fd=0.5, fr=100, ov=0.25, geo=(50, 25, 38), T=(100, 5000, 5121, 8000, 16123, 40000)),
    "ov50": dict(fd=0.5, fr=100, ov=0.5, geo=(50, 25, 25), T=(16000, 16123, 40000)),
    "short": dict(fd=0.1, fr=100, ov=0.25, geo=(10, 5, 8), T=(800, 1601, 5000, 5121, 8000), refused=(16000,)),
    "short50": dict(fd=0.1, fr=100, ov=0.5, geo=(10, 5, 5), T=(3000, 5121, 8000, 16000), refused=(16123,)),
    "tworow": dict(fd=0.02, fr=100, ov=0.25, geo=(2, 1, 2), T=(100, 800, 1601), srate=64000),
    "noov": dict(fd=0.5, fr=100, ov=0.0, geo=(50, 25, 50), T=(16000, 16123, 40000)),
    "oddkk": dict(fd=0.5, fr=102, ov=0.25, geo=(51, 26, 38), T=(100, 3000), refused=(5000,)),
    "fr160": dict(fd=1.0, fr=160, ov=0.25, geo=(160, 80, 120), T=(16123, 40000)),
}
BASE_B = (1, 7, 80, 81)
BIG_CASES = ("half", "ov50", "short50")
BIG_B = (246, 247, 630)   # the last count without the large-LDS attribute, the first with it, the last accepted
REFUSED_B = 631           # the first count launch_ola_log refuses
ROW_PARAMS = [(c, B) for c in CASES for B in BASE_B + (BIG_B if c in BIG_CASES else ())]
ROW_IDS = ["%s-B%d" % p for p in ROW_PARAMS]


# ---- geometry, inputs and the reference ---------------------------------------------------------------------
def srate(case):
    return CASES[case].get("srate", 16000)


def samples(case, T):
    return T * srate(case) // 16000


def oracle_config(case, B):
    c = CASES[case]
    return O.FdlpConfig(nfilters=B, coeff_num=10, coeff_range="0,10", order=10, fduration=c["fd"], frate=c["fr"],
                        overlap_fraction=c["ov"], fbank_type="mel,1", srate=srate(case))


def feature_config(case, B):
    from speech_recognition_tools_amd import FeatureConfig
    c = CASES[case]
    return FeatureConfig(nfilters=B, coeff_num=10, coeff_range="0,10", order=10, fduration=c["fd"], frate=c["fr"],
                         overlap_fraction=c["ov"], fbank_type="mel,1", srate=srate(case))


@functools.lru_cache(maxsize=None)
def host_plan(case, B):
    from speech_recognition_tools_amd import FdlpPlan
    return FdlpPlan(feature_config(case, B), device=-1, max_frames=MAX_FRAMES)


def seeded_jitter(case, T, F, attempt=0):
    return np.random.default_rng([list(CASES).index(case), T, attempt]).integers(0, 2, max(F - 1, 0)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def utt_geometry(case, T):
    """(F, L, jitter [F - 1] uint8, ola_plan) of one accepted utterance.  Whether the reference's slicing
    broadcasts can depend on the hop jitter (the drift of its pointer): the jitter is the first seeded stream
    under which ola_plan accepts the length."""
    cfg = oracle_config(case, 1)
    g = O.geometry(cfg)
    F, L = O.n_frames(samples(case, T), g), O.n_out(samples(case, T), cfg)
    for attempt in range(16):
        jit = seeded_jitter(case, T, F, attempt)
        try:
            return F, L, jit, O.ola_plan(F, L, g, [int(v) for v in jit])
        except ValueError:
            continue
    raise AssertionError("no seeded jitter stream under which the oracle accepts %s T = %d" % (case, T))


def refused_geometry(case, T):
    """(F, L, jitter) of a length of the 'refused' column: the first seeded stream under which ola_plan raises."""
    cfg = oracle_config(case, 1)
    g = O.geometry(cfg)
    F, L = O.n_frames(samples(case, T), g), O.n_out(samples(case, T), cfg)
    for attempt in range(16):
        jit = seeded_jitter(case, T, F, attempt)
        try:
            O.ola_plan(F, L, g, [int(v) for v in jit])
        except ValueError as e:
            assert "could not broadcast" in str(e)
            return F, L, jit
    raise AssertionError("no seeded jitter stream under which the oracle refuses %s T = %d" % (case, T))


def cover(case, T):
    """[L] lists of the (frame, envelope column) cells that ola_plan adds into each output row."""
    F, L, _, plan = utt_geometry(case, T)
    rows = [[] for _ in range(L)]
    for i, (dst, src, cnt) in enumerate(plan):
        for q in range(cnt):
            rows[dst + q].append((i, src + q))
    return rows


def tile_spans(case, T, rows_per_tile):
    """Per tile of the utterance: (rows on the tile, frames the kernel's range test puts on it -- dst < t0 + nt
    and dst + kk > t0, a contiguous range because dst does not decrease --, rows that no frame covers)."""
    F, L, _, plan = utt_geometry(case, T)
    kk = CASES[case]["geo"][0]
    cov = cover(case, T)
    out = []
    for t0 in range(0, L, rows_per_tile):
        nt = min(rows_per_tile, L - t0)
        on = [i for i, (dst, _, _) in enumerate(plan) if dst < t0 + nt and dst + kk > t0]
        span = on[-1] - on[0] + 1 if on else 0
        out.append((nt, span, sum(1 for t in range(t0, t0 + nt) if not cov[t])))
    return out


SPECIALS = (np.nan, np.inf, 0.0, -0.0, -3.5, 5e-324, 1e-14, np.nextafter(1e-14, 0.0), 1e300)


@functools.lru_cache(maxsize=None)
def envelopes(case, B, T, special):
    """[F, B, kk] exp(3 N(0, 1)): a wrong frame, band, row or column moves a feature by O(1).  special: NaN in a
    cell of a row two frames overlap (where the case has one), of the first and of the last row of a tile, and
    every value of SPECIALS in three seeded cells that ola_plan reads."""
    F, L, _, _ = utt_geometry(case, T)
    kk = CASES[case]["geo"][0]
    rng = np.random.default_rng([list(CASES).index(case), B, T, int(special)])
    env = np.exp(3.0 * rng.standard_normal((F, B, kk)))
    if special:
        cov = cover(case, T)
        covered = [t for t in range(L) if cov[t]]
        two = [t for t in covered if len(cov[t]) == 2]
        first = [t for t in covered if t % 32 == 0]
        last = [t for t in covered if t % 32 == 31 or t == L - 1]
        for k, rows in enumerate((two, first, last)):
            if rows:
                t = rows[len(rows) // 2]
                i, q = cov[t][-1]
                env[i, (3 * k + 1) % B, q] = np.nan
        for v in SPECIALS:
            for _ in range(3):
                t = covered[int(rng.integers(len(covered)))]
                i, q = cov[t][int(rng.integers(len(cov[t])))]
                env[i, int(rng.integers(B)), q] = v
    env.setflags(write=False)
    return env


@functools.lru_cache(maxsize=None)
def reference(case, B, T, special):
    _, _, jit, _ = utt_geometry(case, T)
    cfg = oracle_config(case, B)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = O.ola_features(envelopes(case, B, T, special), samples(case, T), [int(v) for v in jit], cfg,
                             O.geometry(cfg))
    ref.setflags(write=False)
    return ref


def ulps(y, ref):
    """test_device_log._ulps over the finite cells of ref."""
    fin = np.isfinite(ref)
    u = np.zeros(ref.shape)
    with np.errstate(invalid="ignore"):
        u[fin] = np.abs(y[fin] - ref[fin]) / np.spacing(np.abs(ref[fin]))
    zero = fin & (ref == 0)
    u[zero] = np.abs(y[zero]) / np.finfo(np.float64).tiny
    return u


def expected_f32(v, d):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.rint(v * 10.0 ** d) / 10.0 ** d).astype(np.float32) if d >= 0 else v.astype(np.float32)


def expected_codes(v, d):
    """(int16 codes, flag) of fp64 values v at d >= 0 decimals (include/fdlp.h, ABI 7)."""
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.rint(v * 10.0 ** d)
        ok = np.abs(k) <= 32767          # False for NaN
        q = np.where(ok, np.where(ok, k, 0.0), -32768.0).astype(np.int64)
    q[ok & (k == 0) & np.signbit(k)] = -32768
    return q.astype(np.int16), bool((~ok).any())


def same_bits(a, b):
    """Equal bit for bit outside NaN, NaN in the same cells."""
    ua, ub = a.view(np.uint32 if a.dtype == np.float32 else np.uint64), b.view(
        np.uint32 if b.dtype == np.float32 else np.uint64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(ua[~nan], ub[~nan])


def check_rows(v, f32, q, flag, ref, d, what):
    """The bars of one utterance's rows: v / f32 / q the device's fp64, float32 and code rows (any may be None),
    ref numpy's.  Returns the worst ulp distance."""
    worst = 0.0
    if v is not None:
        assert v.shape == ref.shape, what
        assert np.array_equal(np.isnan(v), np.isnan(ref)), what + ("NaN cells",)
        assert np.array_equal(v == np.inf, ref == np.inf) and not (v == -np.inf).any(), what + ("+inf cells",)
        u = ulps(v, ref)
        worst = float(u.max())
        assert worst <= 1.0, what + (worst, np.unravel_index(np.argmax(u), u.shape))
        if f32 is not None:
            assert same_bits(f32, expected_f32(v, d)), what + ("float32 rows", d)
        if q is not None:
            want_q, _ = expected_codes(v, d)
            assert np.array_equal(q, want_q), what + ("codes", d)
    return worst


# ---- 1. the table reaches every path (CPU) ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lds_thresholds():
    """(last B without the large-LDS attribute, first with it, last accepted, first refused) by bisection over
    ola_info() of host-only plans."""
    def first(key, want):
        lo, hi = 1, 4096   # ola_info(lo)[key] != want, ola_info(hi)[key] == want
        assert host_plan("short", lo).ola_info()[key] != want and host_plan("short", hi).ola_info()[key] == want
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if host_plan("short", mid).ola_info()[key] == want:
                hi = mid
            else:
                lo = mid
        return hi
    a, r = first("needs_attr", True), first("accepted", False)
    return a - 1, a, r - 1, r


def test_table_reaches_every_path():
    from speech_recognition_tools_amd import FdlpError
    classes = {k: set() for k in ("register", "lds_frames", "lds_bands", "no_frame", "one_row", "uncovered")}
    mixed = set()
    for case, c in CASES.items():
        for B in sorted({B for cc, B in ROW_PARAMS if cc == case}):
            plan = host_plan(case, B)
            info = plan.ola_info()
            assert info["accepted"] and info["lds_bytes"] == 8 * info["rows"] * (B + 1)
            assert (plan.kk, int(round(c["fd"] * c["fr"] / 2)), plan.ola_hop) == c["geo"]
            g = O.geometry(oracle_config(case, B))
            assert (g.kk, g.kkb2, g.ola_hop) == c["geo"]
            for T in c["T"]:
                F, L, jit, want = utt_geometry(case, T)
                assert plan.geometry(samples(case, T)) == (F, L) and F >= 1
                if srate(case) != 16000:  # the same frames and rows as the 16 kHz length of the table
                    c16 = O.FdlpConfig(fduration=c["fd"], frate=c["fr"], overlap_fraction=c["ov"])
                    assert (O.n_frames(T, O.geometry(c16)), O.n_out(T, c16)) == (F, L)
                d, s, n = plan.ola_table(samples(case, T), jit)   # the table the kernel is given
                assert [tuple(x) for x in zip(d.tolist(), s.tolist(), n.tolist())] == want
                kinds = set()
                for ti, (nt, span, bare) in enumerate(tile_spans(case, T, info["rows"])):
                    key = (case, B, T, ti)
                    if B > info["reg_bands"]:
                        kind = "lds_bands"
                    elif span > info["reg_frames"]:
                        kind = "lds_frames"
                    else:
                        kind = "register"
                    classes[kind].add(key)
                    kinds.add(kind)
                    if span == 0:
                        classes["no_frame"].add(key)
                    if nt == 1:
                        classes["one_row"].add(key)
                    if bare:
                        classes["uncovered"].add(key)
                if {"register", "lds_frames"} <= kinds:
                    mixed.add((case, B, T))
            assert sum(utt_geometry(case, T)[0] for T in c["T"]) <= MAX_FRAMES
            for T in c.get("refused", ()):
                F, L, jit = refused_geometry(case, T)
                assert plan.geometry(samples(case, T)) == (F, L)
                with pytest.raises(FdlpError, match="reference OLA would fail to broadcast"):
                    plan.ola_table(samples(case, T), jit)
    print({k: len(v) for k, v in classes.items()}, "mixed", sorted(mixed)[:4])
    for k, v in classes.items():
        assert v, k
    assert mixed, "no utterance holds both register and LDS-loop tiles"
    # every class is reached by each case the issue's table lists for it
    assert any(k[0] == "noov" for k in classes["no_frame"]) and any(k[0] == "ov50" for k in mixed)
    assert any(k[0] == "half" and k[2] == 5121 for k in classes["one_row"])
    for case, n in (("short", 5), ("short50", 8)):
        assert max(s for T in CASES[case]["T"] for _, s, _ in tile_spans(case, T, 32)) == n, case
    spans = lambda case: {s for T in CASES[case]["T"] for _, s, _ in tile_spans(case, T, 32)}
    bare = lambda case, T: sum(b for _, _, b in tile_spans(case, T, 32))
    assert spans("recipe") == {1, 2, 3} and bare("recipe", 16000) > 0
    assert utt_geometry("half", 5000)[1] == 32 and utt_geometry("half", 5121)[1] == 33 and bare("half", 5000) > 0
    assert {1, 2, 3, 4} <= spans("ov50")
    assert CASES["tworow"]["geo"][0] == 2 and any(bare("tworow", T) for T in CASES["tworow"]["T"])
    assert all(utt_geometry("oddkk", T)[1] < CASES["oddkk"]["geo"][1] for T in CASES["oddkk"]["T"])
    assert CASES["oddkk"]["geo"][0] % 2 == 1 and CASES["oddkk"]["refused"]
    assert CASES["fr160"]["geo"][0] > 150 and CASES["short"]["refused"] and CASES["short50"]["refused"]
    # the band counts bracket the register path's limit and both LDS thresholds
    info = host_plan("half", 80).ola_info()
    assert (info["rows"], info["reg_frames"], info["reg_bands"]) == (32, 3, 80)
    assert info["reg_bands"] in BASE_B and info["reg_bands"] + 1 in BASE_B
    assert lds_thresholds() == (BIG_B[0], BIG_B[1], BIG_B[2], REFUSED_B)
    for case in BIG_CASES:
        assert [host_plan(case, B).ola_info()["needs_attr"] for B in BIG_B] == [False, True, True]
        refused = host_plan(case, REFUSED_B).ola_info()
        assert not refused["accepted"] and refused["needs_attr"]


# ---- 2. the reference (CPU) -----------------------------------------------------------------------------------
def test_reference_is_the_oracles_last_lines():
    import random
    meta, sig, _, _ = load_golden("cli_default_mel")
    cfg = oracle_cfg(meta)
    orc = O.FdlpOracle(cfg)
    x = sig[meta["utts"][0]]
    keep = O.Intermediates()
    want = orc.utterance(x, random.Random(9), keep)
    rng = random.Random(9)
    jit = [rng.randrange(2) for _ in range(keep.env.shape[0] - 1)]
    got = O.ola_features(keep.env, x.size, jit, cfg, orc.g)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_reference_sums_have_at_most_two_terms():
    """The premise of the 1-ulp bar: two-term fp64 sums do not depend on their order."""
    deepest = 0
    for case, c in CASES.items():
        for T in c["T"]:
            deepest = max(deepest, max(len(r) for r in cover(case, T)))
            assert max(len(r) for r in cover(case, T)) <= 2, (case, T)
    assert deepest == 2


# ---- GPU --------------------------------------------------------------------------------------------------------
_PLANS = {}


def device_plan(case, B):
    from speech_recognition_tools_amd import FdlpPlan
    if (case, B) not in _PLANS:
        _PLANS[(case, B)] = FdlpPlan(feature_config(case, B), device=0, max_frames=MAX_FRAMES)
    return _PLANS[(case, B)]


@pytest.fixture(scope="module", autouse=True)
def _close_plans():
    yield
    for p in _PLANS.values():
        p.close()
    _PLANS.clear()


def layout(case, Ts):
    """First rows of the utterances, placed in reverse order with gaps of 1 and 33 rows (one in front, 33 behind
    the last), and the buffer's row count."""
    rows, at = {}, 1
    for n, T in enumerate(reversed(Ts)):
        rows[T] = at
        at += utt_geometry(case, T)[1] + (33 if n % 2 == 0 else 1)
    return [rows[T] for T in Ts], at


def launch(case, B, Ts, d, special=False, envs=None, f64=True, f32=True, codes=True, rows=None, total=None):
    """One fdlp_ola_rows launch of the utterances Ts into sentinel-filled buffers: (fp64, float32, codes) host
    arrays (None where not requested), the flag and the first rows."""
    import torch
    plan = device_plan(case, B)
    if rows is None:
        rows, total = layout(case, Ts)
    envs = envs if envs is not None else [envelopes(case, B, T, special) for T in Ts]
    env = torch.from_numpy(np.concatenate(envs) if envs else np.zeros((0, B, plan.kk))).cuda()
    jit = np.concatenate([utt_geometry(case, T)[2] for T in Ts] + [np.zeros(1, np.uint8)])
    o64 = torch.full((total, B), SENT64, dtype=torch.float64, device="cuda") if f64 else None
    o32 = torch.full((total, B), float(SENT32), dtype=torch.float32, device="cuda") if f32 else None
    oq = torch.full((total, B), SENTQ, dtype=torch.int16, device="cuda") if codes else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda") if codes else None
    plan.ola_rows(env, [samples(case, T) for T in Ts], jit, out_rows=rows, ark_decimals=d, want_f64=False, out=o32,
                  out_q=oq, q_flag=flag, out_f64=o64)
    torch.cuda.synchronize()
    host = [t.cpu().numpy() if t is not None else None for t in (o64, o32, oq)]
    return host, (int(flag.item()) if codes else None), rows


def outside_keeps_sentinel(case, Ts, rows, bufs):
    inside = np.zeros(bufs[0].shape[0] if bufs[0] is not None else bufs[2].shape[0], dtype=bool)
    for T, r in zip(Ts, rows):
        assert not inside[r:r + utt_geometry(case, T)[1]].any()   # the layout does not overlap
        inside[r:r + utt_geometry(case, T)[1]] = True
    return all(b is None or (b[~inside] == s).all() for b, s in zip(bufs, (SENT64, SENT32, SENTQ))) and (~inside).any()


def measure_rows(case, B, decimals=DECIMALS, sets=(False, True)):
    """test_rows_against_reference's launches and assertions; returns the worst ulp distance."""
    Ts = CASES[case]["T"]
    worst = 0.0
    for special in sets:
        for d in decimals:
            (v, f32, q), flag, rows = launch(case, B, Ts, d, special, codes=d >= 0)
            what = (case, B, d, special)
            assert outside_keeps_sentinel(case, Ts, rows, (v, f32, q)), what
            no_code = False
            for T, r in zip(Ts, rows):
                L = utt_geometry(case, T)[1]
                cut = [a[r:r + L] if a is not None else None for a in (v, f32, q)]
                worst = max(worst, check_rows(cut[0], cut[1], cut[2], flag, reference(case, B, T, special), d,
                                              what + (T,)))
                if d >= 0:
                    no_code |= expected_codes(cut[0], d)[1]
            if d >= 0:
                assert (flag != 0) == no_code, what + ("flag", flag)
                (_, _, q2), flag2, _ = launch(case, B, Ts, d, special, f64=False, f32=False)   # the codes alone
                assert np.array_equal(q2, q) and (flag2 != 0) == no_code, what + ("codes alone",)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case,B", ROW_PARAMS, ids=ROW_IDS)
def test_rows_against_reference(case, B):
    worst = measure_rows(case, B)
    print("ola stage %s B %d: worst %.3f ulp" % (case, B, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_an_utterance_does_not_depend_on_its_batch(case):
    """Each utterance alone equals, bit for bit, itself inside the batch, inside the reversed batch and inside a
    batch whose other utterances' envelopes are all NaN (nothing of a neighbour is read)."""
    Ts = CASES[case]["T"]
    for B in (7, 81):
        for T in Ts:
            alone, flag, _ = launch(case, B, [T], 3)
            L = utt_geometry(case, T)[1]
            alone = [a[1:1 + L] for a in alone]
            others_nan = [envelopes(case, B, t, False) if t == T else np.full_like(envelopes(case, B, t, False), np.nan)
                          for t in Ts]
            for order, envs in ((Ts, None), (Ts[::-1], None), (Ts, others_nan)):
                got, _, rows = launch(case, B, list(order), 3, envs=envs)
                r = rows[list(order).index(T)]
                for a, b in zip(alone, got):
                    assert a.tobytes() == b[r:r + L].tobytes(), (case, B, T, order == Ts, envs is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_refusals(case):
    import torch
    from speech_recognition_tools_amd import FdlpError
    B = 7
    plan = device_plan(case, B)
    ok_T = CASES[case]["T"][0]
    for T in CASES[case].get("refused", ()):
        F, L, jit_bad = refused_geometry(case, T)
        Fo, Lo, jit_ok = utt_geometry(case, ok_T)[:3]
        env = torch.ones((Fo + F, B, plan.kk), dtype=torch.float64, device="cuda")
        bufs = [torch.full((Lo + L + 2, B), s, dtype=dt, device="cuda")
                for s, dt in ((float(SENT32), torch.float32), (SENT64, torch.float64), (SENTQ, torch.int16))]
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(FdlpError, match="reference OLA would fail to broadcast"):
            plan.ola_rows(env, [samples(case, ok_T), samples(case, T)], np.concatenate([jit_ok, jit_bad]), out=bufs[0],
                          out_f64=bufs[1], out_q=bufs[2], q_flag=flag, want_f64=False)
        torch.cuda.synchronize()
        for b, s in zip(bufs, (SENT32, SENT64, SENTQ)):
            assert (b.cpu().numpy() == s).all(), (case, T)
        assert int(flag.item()) == 0
    # no utterance: succeeds and writes nothing
    (v, f32, q), flag, _ = launch(case, B, [], 3, rows=[], total=4)
    assert (v == SENT64).all() and (f32 == SENT32).all() and (q == SENTQ).all() and flag == 0
    # codes need decimals and a flag
    env = torch.from_numpy(envelopes(case, B, ok_T, False).copy()).cuda()
    L = utt_geometry(case, ok_T)[1]
    oq = torch.full((L, B), SENTQ, dtype=torch.int16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    jit = utt_geometry(case, ok_T)[2]
    with pytest.raises(FdlpError, match="ark_decimals >= 0"):
        plan.ola_rows(env, [samples(case, ok_T)], jit, ark_decimals=-1, want_f64=False, out_q=oq, q_flag=flag)
    with pytest.raises(FdlpError, match="out_q_flag_dev"):
        plan.ola_rows(env, [samples(case, ok_T)], jit, ark_decimals=3, want_f64=False, out_q=oq, q_flag=None)
    torch.cuda.synchronize()
    assert (oq.cpu().numpy() == SENTQ).all()
    with pytest.raises(FdlpError, match="host-only"):
        host_plan(case, B).ola_rows(env, [samples(case, ok_T)], jit)


@pytest.mark.gpu
@pytest.mark.parametrize("case", BIG_CASES)
def test_first_refused_band_count(case):
    """REFUSED_B bands: plan creation accepts them, launch_ola_log's host test refuses the launch with an error
    code, and nothing is written."""
    import torch
    from speech_recognition_tools_amd import FdlpError, FdlpPlan
    plan = FdlpPlan(feature_config(case, REFUSED_B), device=0, max_frames=MAX_FRAMES)
    T = CASES[case]["T"][0]
    F, L, jit, _ = utt_geometry(case, T)
    env = torch.ones((F, REFUSED_B, plan.kk), dtype=torch.float64, device="cuda")
    bufs = [torch.full((L, REFUSED_B), s, dtype=dt, device="cuda")
            for s, dt in ((float(SENT32), torch.float32), (SENT64, torch.float64), (SENTQ, torch.int16))]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(FdlpError) as e:
        plan.ola_rows(env, [samples(case, T)], jit, out=bufs[0], out_f64=bufs[1], out_q=bufs[2], q_flag=flag,
                      want_f64=False)
    assert e.value.code < 0 and "launch_ola_log" in str(e.value)
    torch.cuda.synchronize()
    for b, s in zip(bufs, (SENT32, SENT64, SENTQ)):
        assert (b.cpu().numpy() == s).all()
    plan.close()


PIPELINE_CASES = [(c, B) for c in ("ov50", "short", "noov") for B in (7, 81)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,B", PIPELINE_CASES, ids=["%s-B%d" % p for p in PIPELINE_CASES])
def test_entry_point_is_the_production_path(case, B):
    """fdlp_compute on seeded int16 noise, its envelopes fetched, fdlp_ola_rows on them: the same fp64 rows,
    float32 rows and codes bit for bit, and those rows within the bars against numpy on the fetched envelopes."""
    import torch
    plan = device_plan(case, B)
    Ts = CASES[case]["T"]
    lens = [samples(case, T) for T in Ts]
    rng = np.random.default_rng([list(CASES).index(case), B])
    pcm = np.clip(np.round(rng.standard_normal(sum(lens)) * 3000), -32768, 32767).astype(np.int16)
    jit = np.concatenate([utt_geometry(case, T)[2] for T in Ts])
    total = sum(utt_geometry(case, T)[1] for T in Ts)
    nf = sum(utt_geometry(case, T)[0] for T in Ts)
    oq = torch.full((total, B), SENTQ, dtype=torch.int16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((total, B), float(SENT32), dtype=torch.float32, device="cuda")
    out, rows, out64 = plan.compute(torch.from_numpy(pcm).cuda(), lens, jit, want_f64=True, out=out, out_q=oq,
                                    q_flag=flag)
    torch.cuda.synchronize()
    env = plan.debug_fetch(nf, keys=("env",))["env"]
    assert np.isfinite(env).all() and (env >= 0).all() and (env[..., 1:-1] > 0).all()  # hanning(kk) ends in 0
    oq2 = torch.full((total, B), SENTQ, dtype=torch.int16, device="cuda")
    flag2 = torch.zeros(1, dtype=torch.int32, device="cuda")
    out2 = torch.full((total, B), float(SENT32), dtype=torch.float32, device="cuda")
    f32, rows2, f64 = plan.ola_rows(torch.from_numpy(env).cuda(), lens, jit, out=out2, out_q=oq2, q_flag=flag2)
    torch.cuda.synchronize()
    assert rows2.tolist() == rows[:-1].tolist()
    v = out64.cpu().numpy()
    assert f64.cpu().numpy().tobytes() == v.tobytes()
    assert f32.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
    assert oq2.cpu().numpy().tobytes() == oq.cpu().numpy().tobytes() and int(flag2.item()) == int(flag.item())
    cfg = oracle_config(case, B)
    f0 = 0
    for T, r in zip(Ts, rows[:-1]):
        F, L, j, _ = utt_geometry(case, T)
        ref = O.ola_features(env[f0:f0 + F], samples(case, T), [int(x) for x in j], cfg, O.geometry(cfg))
        check_rows(v[r:r + L], out.cpu().numpy()[r:r + L], oq.cpu().numpy()[r:r + L], None, ref, 3, (case, B, T))
        f0 += F
    assert (int(flag.item()) != 0) == expected_codes(v, 3)[1]


# ---- the range-check build ---------------------------------------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import torch
import test_ola_stage as T
from speech_recognition_tools_amd.plan import device_checks
assert device_checks(reset=True)[0], "not a checks build"
runs = 0
for case, B in T.ROW_PARAMS:
    T.measure_rows(case, B, decimals=(3,))
    runs += 1
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": runs}))
"""


@pytest.mark.gpu
def test_rows_under_range_checks():
    """test_rows_against_reference's launches, once each at ark_decimals 3, through the library built with
    -DFDLP_DEVICE_CHECKS=1 (one child process: the library is chosen when it is loaded): the tile index, the
    register path's clamped frame index, envelope column and LDS cell, the LDS loop's envelope column and the
    store loop's row / band split stay inside their ranges."""
    assert os.path.exists(CHECKS_LIB), "build() compiles libfdlp_checks.so"
    env = dict(os.environ, FDLP_LIB=CHECKS_LIB)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["enabled"] and res["runs"] == len(ROW_PARAMS)
    assert res["violations"] == 0, res
