"""Every xform_kernel instantiation held to the fmaf chain include/fdlp.h documents for it.

launch_xform (csrc/fdlp_post.hip) picks one of 16 code objects xform_kernel<MODE, NCB>, each of which branches over six
forms of xform_chunk<TWO, FULL, VEC>, loops over column groups of 16 NCB and runs on a tile of 128, 64, .., 1 frames
(the last one possibly above 64 KB of dynamic LDS).  XformPlan.dispatch() reports which of these a plan takes, from
the function the launcher itself selects by; test_cases_reach_their_hazards holds the table below to all of them.

The twin.  The header promises, for a row `a` entering the transform and matrix row `m`,

    acc = +0;  for g = 0, 16, ..: for s = 0 .. 3: for q = 0 .. 3: k = g + 4 q + s (< K): acc = fmaf(a[k], m[k], acc)

and then (affine) one float32 add of m[K].  The matrices of test_gpu_chain_bits hold only +-2^e, e in [-3, 3]: then
a[k] m[k] is exact in float32 (the rows are far from the overflow and underflow thresholds), so
np.float32(acc + np.float32(a * m)) rounds once, as fmaf does, and a plain numpy float32 loop over k IS the promise,
bit for bit, for arbitrary rows.  The rows are the device's own PostPlan output, which tests/test_post.py holds to
numpy.  A case with K >= 32 also has to tell the documented order from the natural one k = 0, 1, 2, ..: the twin in
natural order must differ somewhere, or the case would prove nothing about the order.

The fused-against-chained test uses real-valued matrices (test_transform.make_mat) and needs no twin: the fused
launch of every (MODE >= 0, NCB) must give the bits of the stand-alone transform (MODE -1, same NCB) on PostPlan's
rows, and stay within test_transform.ref_and_bound where K <= 4096."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import post_numpy as PN
import test_transform as TT
from conftest import ROOT

# lengths whose last tile under tile 128 has 1, 15, 16, 17, 63, 64, 65, 80, 81 and 127 rows: the four waves of a
# workgroup then differ in act0 / act1, and TWO is on and off within one launch
LAST_ROWS_128 = (1, 15, 16, 17, 63, 64, 65, 80, 81, 127)
LENS_128 = (1, 15, 16, 17, 63, 64, 65, 80, 81, 127, 128 + 17, 128)


def lens_for(tile):
    """tile - 1, tile, tile + 1, 2 tile + 3 and 1 under a tile below 128"""
    return LENS_128 if tile == 128 else tuple(sorted({T for T in (1, tile - 1, tile, tile + 1, 2 * tile + 3) if T >= 1}))


# K of the stand-alone transform (every stage off, dim = K): K % 32 in {0, 1, 3, 4, 5, 15, 16, 17, 20, 31}, K < 32 on
# its own, K = 32 and K = 33
TAIL_KS = (5, 31, 32, 33, 35, 36, 37, 47, 48, 49, 52, 63, 64)
TAILS = (0, 1, 3, 4, 5, 15, 16, 17, 20, 31)
NS_OF_NCB = {1: (1, 9, 16), 2: (17, 25, 32), 3: (33, 40, 48), 4: (49, 57, 64)}

# (D, order, window, L, R, N, affine, lengths)
CASES = []
for _i, _K in enumerate(TAIL_KS):
    for _ncb in (1, 2, 3, 4):
        CASES.append((_K, 0, 2, 0, 0, NS_OF_NCB[_ncb][(_i + _ncb) % 3], bool((_i + _ncb) % 2), LENS_128))
CASES += [
    # column groups without deltas: one full group, a second group of one column, two full groups, 130
    (37, 0, 2, 0, 0, 64, True, LENS_128), (37, 0, 2, 0, 0, 65, False, LENS_128),
    (64, 0, 2, 0, 0, 128, True, LENS_128), (13, 0, 2, 2, 2, 130, True, LENS_128),
    # mode 0: a window other than 2, and order 3 at window 2
    (13, 2, 3, 1, 1, 9, True, LENS_128),       # ncb 1, K = 117, scalar LDS reads
    (8, 3, 2, 2, 1, 32, False, LENS_128),      # ncb 2, K = 128, 16-byte reads
    (5, 1, 1, 3, 0, 48, True, LENS_128),       # ncb 3, K = 40
    (10, 3, 2, 1, 1, 65, False, LENS_128),     # ncb 4, K = 120, a second column group
    (80, 3, 2, 5, 5, 33, True, lens_for(16)),  # K = 3520, tile 16
    # mode 1: order 1 at window 2
    (13, 1, 2, 2, 2, 16, False, LENS_128),     # ncb 1, K = 130, scalar
    (14, 1, 2, 1, 1, 17, True, LENS_128),      # ncb 2, K = 84, 16-byte
    (7, 1, 2, 3, 1, 40, False, LENS_128),      # ncb 3, K = 70, scalar
    (20, 1, 2, 1, 0, 130, True, LENS_128),     # ncb 4, K = 80, three column groups
    # mode 2: order 2 at window 2
    (13, 2, 2, 4, 4, 1, True, LENS_128),       # ncb 1, K = 351, scalar
    (4, 2, 2, 2, 2, 32, False, LENS_128),      # ncb 2, K = 60, 16-byte
    (13, 2, 2, 1, 1, 40, True, LENS_128),      # ncb 3, K = 117, scalar
    (12, 2, 2, 1, 1, 128, False, LENS_128),    # ncb 4, K = 108, two column groups
    (40, 2, 2, 4, 4, 70, True, lens_for(64)),      # K = 1080, tile 64
    (80, 2, 2, 4, 4, 17, False, lens_for(32)),     # K = 2160, tile 32
    (80, 2, 2, 10, 10, 65, True, lens_for(8)),     # K = 5040, tile 8
    (120, 2, 2, 10, 10, 48, False, lens_for(4)),   # K = 7560, tile 4
    (300, 2, 2, 3, 3, 64, True, lens_for(2)),      # K = 6300, tile 2
    (80, 2, 2, 20, 20, 40, False, lens_for(1)),    # K = 9840, tile 1 at 68352 bytes
    (440, 2, 2, 4, 4, 17, True, lens_for(1)),      # K = 11880, tile 1 at 86656 bytes
    (200, 2, 2, 8, 8, 130, False, lens_for(1)),    # K = 10200, tile 1 at 78208 bytes, three column groups
    # above 64 KB in the other three modes, and scalar LDS reads at small tiles
    (601, 0, 2, 16, 15, 7, True, lens_for(1)),     # mode -1, K = 19232, tile 1 at 82048 bytes, scalar
    (450, 1, 1, 10, 10, 33, True, lens_for(1)),    # mode 0, K = 18900, tile 1 at 130320 bytes
    (350, 1, 2, 8, 8, 64, False, lens_for(1)),     # mode 1, K = 11900, tile 1 at 94416 bytes
    (333, 1, 2, 5, 4, 50, False, lens_for(1)),     # mode 1, K = 6660, tile 1 below 64 KB, scalar
    (81, 2, 2, 10, 10, 20, True, lens_for(16)),    # mode 2, K = 5103, tile 16, scalar
]
CASE_IDS = ["D%d-o%dw%d-L%dR%d-N%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "a" if c[6] else "") for c in CASES]
ALL_PAIRS = {(m, n) for m in (-1, 0, 1, 2) for n in (1, 2, 3, 4)}


def case_cfg(case):
    from speech_recognition_tools_amd.post import PostConfig
    D, order, window, L, R = case[:5]
    return PostConfig(dim=D, delta_order=order, delta_window=window, left_context=L, right_context=R)


def host_dispatch(case):
    from speech_recognition_tools_amd.post import XformPlan
    p = XformPlan(case_cfg(case), case[5], case[6], device=-1)
    d = p.dispatch()
    d["K"], d["lds_bytes"] = p.in_dim, p.lds_bytes
    return d


def chain_order(K):
    """the k of the documented chain, in the order it visits them"""
    return [g + 4 * q + s for g in range(0, K, 16) for s in range(4) for q in range(4) if g + 4 * q + s < K]


def chain_twin(A, M, order):
    """float32 [rows, N]: acc = fl(acc + A[:, k] M[:, k]) over k in `order` from +0, then one add of the offset column.
    Each step is one float32 rounding, which is fmaf's when the product is exact (module docstring)."""
    K = A.shape[1]
    assert A.dtype == np.float32 and M.dtype == np.float32 and M.shape[1] in (K, K + 1) and sorted(order) == list(range(K))
    Mt = np.ascontiguousarray(M.T)
    acc = np.zeros((A.shape[0], M.shape[0]), dtype=np.float32)
    for k in order:
        acc += A[:, k, None] * Mt[k][None, :]
    if M.shape[1] == K + 1:
        acc += Mt[K][None, :]
    assert acc.dtype == np.float32
    return acc


def pow2_mat(rng, N, K, affine):
    """+-2^e, e in [-3, 3]; the offset column (affine) an arbitrary float32"""
    m = (np.ldexp(1.0, rng.integers(-3, 4, (N, K + int(affine)))) * rng.choice([-1.0, 1.0], (N, K + int(affine))))
    if affine:
        m[:, K] = rng.standard_normal(N) * 3.0
    return m.astype(np.float32)


def build_case(case, seed, make_mat=pow2_mat):
    """utterances, the two CMVN pairs and their index, two matrices and a mat_index out of step with it"""
    D, order, window, L, R, N, affine, lens = case
    rng = np.random.default_rng(seed)
    xs = [TT.ark_like(rng, T, D, 2.0 * (i % 2)) for i, T in enumerate(lens)]
    norms = [PN.cmvn_norm(TT.stats_of(np.concatenate(xs[k::2] or xs)), norm_vars=True) for k in (0, 1)]
    idx = [i % 2 for i in range(len(xs))]
    K = D * (order + 1) * (L + R + 1)
    mats = [make_mat(rng, N, K, affine) for _ in range(2)]
    midx = [(i // 2) % 2 for i in range(len(xs))]
    return xs, norms, idx, mats, midx


def case_seed(i):
    return 7000 + i


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_cases_reach_their_hazards():
    """CPU: from dispatch() on host-only plans, the table reaches every instantiation, branch, column-group count and
    tile this module's docstring names."""
    disp = [host_dispatch(c) for c in CASES]
    for c, d in zip(CASES, disp):
        D, order, window, L, R, N, affine, lens = c
        K = D * (order + 1) * (L + R + 1)
        assert d["K"] == K == 32 * d["full_chunks"] + d["tail"] and 0 <= d["tail"] < 32, c
        assert d["ncb"] == min((N + 15) // 16, 4) and d["groups"] == -(-N // (16 * d["ncb"])), c
        assert d["vec"] == ((D * (order + 1)) % 4 == 0) and d["big_lds"] == (d["lds_bytes"] > 65536), c
        want_mode = -1 if order == 0 else (order if window == 2 and order <= 2 else 0)
        assert d["mode"] == want_mode, c
        # the lengths put the tile's edges into the launch
        if d["tile"] == 128:
            assert {(T - 1) % 128 + 1 for T in lens} >= set(LAST_ROWS_128) and max(lens) > 128, c
        else:
            assert set(lens) >= set(lens_for(d["tile"])), (c, d["tile"])
        assert not d["big_lds"] or d["tile"] == 1, c
    assert {(d["mode"], d["ncb"]) for d in disp} == ALL_PAIRS
    assert {(d["mode"], d["vec"]) for d in disp} == {(m, v) for m in (-1, 0, 1, 2) for v in (False, True)}
    # mode 0 from a window other than 2 and from order 3 at window 2
    assert any(d["mode"] == 0 and c[2] != 2 for c, d in zip(CASES, disp))
    assert any(d["mode"] == 0 and c[1:3] == (3, 2) for c, d in zip(CASES, disp))
    # K tails and sizes of the stand-alone transform, at each NCB
    alone = [(c, d) for c, d in zip(CASES, disp) if c[1:5] == (0, 2, 0, 0)]
    for ncb in (1, 2, 3, 4):
        ks = {d["K"] for c, d in alone if d["ncb"] == ncb and d["groups"] == 1}
        assert {k % 32 for k in ks if k > 32} >= set(TAILS) - {0} and {32, 33, 64} <= ks and any(k < 32 for k in ks), ncb
        assert all(d["mode"] == -1 and d["tile"] == 128 for c, d in alone if d["ncb"] == ncb)
    # column groups
    by_n = {c[5]: d for c, d in zip(CASES, disp) if d["mode"] == -1}
    assert [(by_n[n]["ncb"], by_n[n]["groups"]) for n in (64, 65, 128, 130)] == [(4, 1), (4, 2), (4, 2), (4, 3)]
    for mode in (0, 1, 2):
        assert any(d["mode"] == mode and d["groups"] > 1 and c[5] in (65, 128, 130) for c, d in zip(CASES, disp)), mode
    # tiles, and one frame per tile above 64 KB
    assert {d["tile"] for d in disp} == {128, 64, 32, 16, 8, 4, 2, 1}
    big = [(c[:6], d["K"], d["lds_bytes"]) for c, d in zip(CASES, disp) if d["big_lds"]]
    assert big[:3] == [((80, 2, 2, 20, 20, 40), 9840, 68352), ((440, 2, 2, 4, 4, 17), 11880, 86656),
                       ((200, 2, 2, 8, 8, 130), 10200, 78208)]
    assert {d["mode"] for d in disp if d["big_lds"]} == {-1, 0, 1, 2}
    assert any(d["tile"] < 16 and d["groups"] > 1 for d in disp) and any(d["tile"] < 16 and not d["vec"] for d in disp)
    assert len(set(CASE_IDS)) == len(CASES)


def test_twin_is_the_fmaf_chain_and_shows_the_order():
    """CPU: with a +-2^e matrix the float32 loop equals the chain evaluated in exact rational arithmetic and rounded
    once per k (what fmaf does), and the natural order gives other bits."""
    from fractions import Fraction
    rng = np.random.default_rng(117)
    K, N = 117, 3
    A = TT.ark_like(rng, 4, K, 1.0)
    M = pow2_mat(rng, N, K, True)
    got = chain_twin(A, M, chain_order(K))
    for r in range(A.shape[0]):
        for n in range(N):
            acc = np.float32(0)
            for k in chain_order(K):
                exact = Fraction(float(A[r, k])) * Fraction(float(M[n, k])) + Fraction(float(acc))
                f64 = float(exact)
                assert Fraction(f64) == exact    # it fits a double, so the conversion below is the one rounding
                acc = np.float32(f64)
            acc = np.float32(np.float64(acc) + np.float64(M[n, K]))
            assert acc.view(np.uint32) == got[r, n].view(np.uint32), (r, n)
    assert not np.array_equal(TT.bits(got), TT.bits(chain_twin(A, M, list(range(K)))))
    assert chain_order(37) == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15,
                               16, 20, 24, 28, 17, 21, 25, 29, 18, 22, 26, 30, 19, 23, 27, 31, 32, 36, 33, 34, 35]


def test_dispatch_is_declared_and_refuses_null():
    import ctypes
    from speech_recognition_tools_amd import _lib
    from speech_recognition_tools_amd._lib import FdlpError, check
    from speech_recognition_tools_amd.post import PostConfig, XformPlan
    src = open(os.path.join(ROOT, "include", "fdlp.h")).read()
    assert "int fdlp_xform_plan_dispatch(const fdlp_xform_plan* plan, int32_t info[8]);" in src
    assert "fdlp_xform_plan_dispatch" in _lib.SIGNATURES and hasattr(_lib.lib, "fdlp_xform_plan_dispatch")
    p = XformPlan(PostConfig(dim=13), 13, True, device=-1)
    assert p.dispatch() == dict(mode=-1, ncb=1, groups=1, tile=128, vec=False, full_chunks=0, tail=13, big_lds=False)
    with pytest.raises(FdlpError):
        check(_lib.lib.fdlp_xform_plan_dispatch(None, (ctypes.c_int32 * 8)()))
    with pytest.raises(FdlpError):
        check(_lib.lib.fdlp_xform_plan_dispatch(p._h, None))
    # the launcher selects by the report's function, and the mode expression is written once
    hip = open(os.path.join(ROOT, "speech_recognition_tools_amd", "csrc", "fdlp_post.hip")).read()
    assert hip.count("kPostSpecWindow && ") == 1 and hip.count("xform_dispatch(c, xc.N)") == 1


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_gpu_chain_bits(ci):
    """the fused output is the documented chain on the device's own PostPlan rows, bit for bit"""
    from speech_recognition_tools_amd.post import PostPlan, XformPlan
    case = CASES[ci]
    N, affine = case[5], case[6]
    cfg = case_cfg(case)
    plan = XformPlan(cfg, N, affine)
    d = plan.dispatch()
    assert d == {k: v for k, v in host_dispatch(case).items() if k in d}
    xs, norms, idx, mats, midx = build_case(case, case_seed(ci))
    got = TT.run_xform(plan, xs, mats, midx, norms, idx)
    rows = TT.run_post(PostPlan(cfg), xs, norms, idx)
    K = plan.in_dim
    assert got.shape == (rows.shape[0], N) and rows.shape[1] == K
    order = chain_order(K)
    bad = differs = 0
    for g, A, m in zip(TT.split_rows(got, xs), TT.split_rows(rows, xs), midx):
        A = np.ascontiguousarray(A)
        twin = chain_twin(A, mats[m], order)
        bad += int((TT.bits(g) != TT.bits(twin)).sum())
        if K >= 32:
            differs += int((TT.bits(twin) != TT.bits(chain_twin(A, mats[m], list(range(K))))).sum())
    print("xform_kernel<%d,%d> groups %d tile %d vec %d K %d = 32*%d + %d lds %d%s rows %d: %d of %d elements differ "
          "from the documented chain; natural order differs in %d"
          % (d["mode"], d["ncb"], d["groups"], d["tile"], d["vec"], K, d["full_chunks"], d["tail"], plan.lds_bytes,
             " (>64K)" if d["big_lds"] else "", got.shape[0], bad, got.size, differs))
    assert K < 32 or differs > 0, "the data does not show the order"
    assert bad == 0


def fused_cases():
    """one table row per fused (mode >= 0, ncb) instantiation, the smallest K first"""
    pick = {}
    for ci, c in enumerate(CASES):
        if c[1] == 0:
            continue
        window, order, N = c[2], c[1], c[5]
        key = (order if window == 2 and order <= 2 else 0, min((N + 15) // 16, 4))
        K = c[0] * (order + 1) * (c[3] + c[4] + 1)
        if key not in pick or K < pick[key][0]:
            pick[key] = (K, ci)
    return [pick[k][1] for k in sorted(pick)]


FUSED = fused_cases()


def test_fused_cases_are_the_twelve():
    disp = [host_dispatch(CASES[ci]) for ci in FUSED]
    assert sorted((d["mode"], d["ncb"]) for d in disp) == sorted(p for p in ALL_PAIRS if p[0] >= 0)
    assert all(d["K"] <= 4096 for d in disp)


@pytest.mark.gpu
@pytest.mark.parametrize("ci", FUSED, ids=[CASE_IDS[ci] for ci in FUSED])
def test_gpu_fused_equals_chained_every_mode(ci):
    """fused launch = PostPlan to HBM, then the stand-alone transform (mode -1, same NCB), bit for bit"""
    import torch
    from speech_recognition_tools_amd.post import PostConfig, PostPlan, XformPlan
    case = CASES[ci]
    N, affine = case[5], case[6]
    cfg = case_cfg(case)
    plan = XformPlan(cfg, N, affine)
    d = plan.dispatch()
    K = plan.in_dim
    xs, norms, idx, mats, midx = build_case(case, case_seed(ci), TT.make_mat)
    fused = TT.run_xform(plan, xs, mats, midx, norms, idx)
    rows = TT.run_post(PostPlan(cfg), xs, norms, idx)
    alone = XformPlan(PostConfig(dim=K), N, affine)
    da = alone.dispatch()
    assert d["mode"] >= 0 and (da["mode"], da["ncb"], da["groups"]) == (-1, d["ncb"], d["groups"])
    lens = [x.shape[0] for x in xs]
    chained = alone.compute(torch.from_numpy(rows).cuda(), lens, torch.from_numpy(np.stack(mats)).cuda(), midx)
    torch.cuda.synchronize()
    print("xform_kernel<%d,%d> tile %d against xform_kernel<-1,%d> tile %d, K %d" % (d["mode"], d["ncb"], d["tile"],
                                                                                     da["ncb"], da["tile"], K))
    TT.assert_bits_equal(fused, chained.cpu().numpy(), CASE_IDS[ci])
    if K <= 4096:
        for g, A, m in zip(TT.split_rows(fused, xs), TT.split_rows(rows, xs), midx):
            TT.assert_within_bound(g, A, mats[m], CASE_IDS[ci])


CHECKS_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import test_transform as TT
import test_xform_dispatch as XD
from speech_recognition_tools_amd.plan import device_checks
from speech_recognition_tools_amd.post import XformPlan
assert device_checks(reset=True)[0], "not a checks build"
runs = 0
for ci, case in enumerate(XD.CASES):
    plan = XformPlan(XD.case_cfg(case), case[5], case[6])
    xs, norms, idx, mats, midx = XD.build_case(case, XD.case_seed(ci))
    got = TT.run_xform(plan, xs, mats, midx, norms, idx)
    assert np.all(np.isfinite(got)), case
    runs += 1
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": runs}))
"""


@pytest.mark.gpu
def test_gpu_device_range_checks_silent_over_the_table():
    """the FDLP_DEVICE_CHECKS build: LDS, matrix and output indices stay in range at every instantiation and tile"""
    lib = os.path.join(ROOT, "speech_recognition_tools_amd", "lib", "libfdlp_checks.so")
    assert os.path.exists(lib), "build() compiles libfdlp_checks.so"
    r = subprocess.run([sys.executable, "-c", CHECKS_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=dict(os.environ, FDLP_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print("range-check build over the table: %s" % json.dumps(res))
    assert res["enabled"] and res["runs"] == len(CASES)
    assert res["violations"] == 0, res
