"""The 2x2 fast-correlation block of ac_vsweep_kernel's plain runs, restated in numpy and walked over the
kernel's own schedule, on integers.

A plain block computes acc[u] += sum_v s[n0+v] W[v+u] (W the lane's window, v, u < A).  In a run the kernel issues
it as three products per 2 positions x 2 lags: for even v, u, with g0 = s[n0+v], g1 = s[n0+v+1],

    Q[u]   += g0        * (W[v+u]   - W[v+u+1])
    M[u/2] += (g0 + g1) *  W[v+u+1]
    Q[u+1] += g1        * (W[v+u+2] - W[v+u+1])

with Q the accumulator itself and M folded into it at the run's end.  Per bank it keeps the signed differences
e[q] (even q: W[q] - W[q+1], odd q: W[q+1] - W[q]; e[A-1] reaches W[0] of the older bank), the raw odd elements and
the raw W[0]; the older bank's differences are reused as they are (A even, block bases multiples of A).  The first
block of a run builds the older bank's differences from the raw bank the general block left, and after the run
that bank is read again raw for the general block that follows.

The walk is plan.sweep_schedule() of host-only plans, the three shapes of test_vsweep_block_order.py (A = 4, 8,
10): runs in the 2x2 form, general blocks by the direct products, split at their events.  The signal is
integer-valued (|s| < 2^10: every product, difference and sum is exact in fp64), so the accumulator at every event,
the sum over the positions consumed so far, must EQUAL the direct truncated autocorrelation: a wrong pairing,
sign, bank or parity cannot hide behind rounding.  (The flat sweep's chains are sums of such accumulators between
events and are not restated; its events are checked as snapshots of the running sum.)"""
import functools

import numpy as np
import pytest

# (fbank_type, nfilters, fduration, order, coeff_num, lags per lane): the shapes of test_vsweep_block_order.py
CFGS = {
    "a4": ("cochlear,2,0.5,1,4,1.2", 20, 0.5, 20, 20, 4),
    "a8": ("cochlear,0.02,1,1,2.5,1", 30, 0.5, 100, 40, 8),
    "a10": ("cochlear,1,1,1,2.5,1", 80, 1.5, 150, 100, 10),
}
# and the one-band shape at the shortest frame of test_vsweep_schedule.py: the three shapes above have a run in every
# sweep; this one's flat sweep is shorter than two blocks (no run) and its lower-skirt sweep is empty
EXTRA = {"one": ("cochlear,1,1,1,2.5,1", 1, 0.064, 10, 10, 4)}
SHAPES = dict(CFGS, **EXTRA)
COMMIT, GENERAL, END = 0, 1, 2
LANES = 16


@functools.lru_cache(maxsize=None)
def _sweeps(tag):
    """(N, nlags, [(name, info, events S in sweep order, records)]) of a host-only plan."""
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig
    fb, nf, fd, order, cn, _ = SHAPES[tag]
    plan = FdlpPlan(FeatureConfig(fbank_type=fb, nfilters=nf, fduration=fd, order=order, coeff_num=cn,
                                  coeff_range="0,%d" % cn), device=-1, max_frames=64)
    chains, parts, ev = plan.flat_events()
    assert chains > 0
    m1, m2 = plan.regions()
    out = []
    for kind, S in ((0, plan.N - m1.astype(np.int64)), (1, m2.astype(np.int64))):
        info, rec = plan.sweep_schedule(kind)
        out.append(("skirt%d" % kind, info, np.sort(S)[::-1], rec))
    k = 0
    for h in range(parts):
        info, rec = plan.sweep_schedule(2, h)
        k1 = len(ev) if h == parts - 1 else k + int((ev[k:, 0] >= info["nlo"]).sum())
        out.append(("flat%d" % h, info, ev[k:k1, 0].astype(np.int64), rec))
        k = k1
    return plan.N, plan.nlags, out


class _Bank:
    """One register bank of every lane: raw (a general block's), or differences, odd elements and W[0] (a run's)."""

    def __init__(self):
        self.raw = self.e = self.od = self.w0 = None


def _walk(s, N, info, S, rec):
    """Walks one sweep; returns ([(S, acc[16 A]) per event], cases met)."""
    A, nlo, nhi = info["A"], info["nlo"], info["nhi"]
    assert A % 2 == 0
    if nhi <= nlo:  # nothing to sweep: every row is zero
        assert rec.tolist() == [[0, END, nlo, len(S)]]
        return [(int(S_k), np.zeros(LANES * A)) for S_k in S], {"empty sweep"}
    sp = np.concatenate([s[:N], np.zeros(20 * A + 32)])  # s is 0 past N
    lanes = np.arange(LANES)
    ev_U = np.arange(0, A, 2)

    def window(n0):  # lane l's new bank: s[n0 + A l + q], q < A
        return sp[n0 + A * lanes[:, None] + np.arange(A)[None, :]]

    acc = np.zeros((LANES, A))
    bank = [_Bank(), _Bank()]  # X, Y
    b_top, b_bot = (nhi - 1) // A, nlo // A
    bank[1].raw = window(A * b_top + A)
    lo_i = 0  # the bank the next block loads: X, then Y, ...
    b, k = b_top, 0
    snaps, met = [], set()

    def direct(n0, lo_p, hi_p):  # positions [lo_p, hi_p) of block n0 by the direct products
        nonlocal lo_i
        lo, hi = bank[lo_i], bank[1 - lo_i]
        assert hi.raw is not None, "a general block needs the older bank raw"
        W = np.concatenate([lo.raw, hi.raw], axis=1)
        for v in range(A):
            if lo_p <= n0 + v < hi_p:
                acc[:, :] += sp[n0 + v] * W[:, v:v + A]

    for run, action, pos, aux in rec.tolist():
        if run:
            assert run % 2 == 0 and lo_i == 0, "runs are whole (X, Y) pairs"
            met.add("run of one pair" if run == 2 else "run")
            # entry: the older bank (Y) from its raw values
            y = bank[1]
            assert y.raw is not None
            y.e = np.where(np.arange(A - 1) % 2 == 1, y.raw[:, 1:] - y.raw[:, :-1], y.raw[:, :-1] - y.raw[:, 1:])
            y.e = np.concatenate([y.e, np.full((LANES, 1), np.nan)], axis=1)  # e[A-1] of the older bank: never used
            y.od, y.w0 = y.raw[:, 1::2].copy(), y.raw[:, 0].copy()
            y.raw = bank[0].raw = None
            M = np.zeros((LANES, A // 2))
            for _ in range(run):
                n0 = A * b
                lo, hi = bank[lo_i], bank[1 - lo_i]
                w = window(n0)
                cur, cur1 = sp[n0 + lanes], sp[n0 + 1 + lanes]
                curs = cur + cur1
                lo.e = np.where(np.arange(A - 1) % 2 == 1, w[:, 1:] - w[:, :-1], w[:, :-1] - w[:, 1:])
                lo.e = np.concatenate([lo.e, (hi.w0 - w[:, A - 1])[:, None]], axis=1)
                lo.od, lo.w0 = w[:, 1::2].copy(), w[:, 0].copy()
                E = np.concatenate([lo.e, hi.e], axis=1)
                OD = np.concatenate([lo.od, hi.od], axis=1)
                for v in range(0, A, 2):
                    acc[:, ev_U] += cur[v] * E[:, v + ev_U]
                    M += curs[v] * OD[:, (v + ev_U + 1) // 2]
                    acc[:, ev_U + 1] += cur[v + 1] * E[:, v + ev_U + 1]
                assert not np.isnan(acc).any()
                lo_i ^= 1
                b -= 1
            acc += np.repeat(M, 2, axis=1)  # the fold: acc[u] += M[u >> 1]
            # exit: the run's last bank (Y again) raw, from the ring
            assert lo_i == 0
            bank[1].raw = window(A * b + A)
            bank[1].e = bank[0].e = None
        if action == COMMIT:
            continue
        if action == GENERAL:
            n0 = A * b
            assert pos == n0
            bank[lo_i].raw = window(n0)
            hi_m = min(n0 + A, nhi)
            for S_k in S[k:k + aux].tolist():
                lo_m = max(S_k, n0, nlo)
                direct(n0, lo_m, hi_m)
                hi_m = min(hi_m, lo_m)
                snaps.append((S_k, acc.reshape(-1).copy()))
            direct(n0, max(n0, nlo), hi_m)
            k += aux
            lo_i ^= 1
            b -= 1
        else:
            for S_k in S[k:k + aux].tolist():
                snaps.append((S_k, acc.reshape(-1).copy()))
            k += aux
    assert k == len(S) and b == b_bot - 1
    if rec[:, 0].max() == 0:
        met.add("sweep with no run")
    return snaps, met


def _truth(s, N, nlo, nhi, S, nl):
    sp = np.concatenate([s[:N], np.zeros(nl)])
    lo = max(S, nlo)
    if lo >= nhi:
        return np.zeros(nl)
    seg = sp[lo:nhi]
    return np.array([np.dot(seg, sp[lo + lag:nhi + lag]) for lag in range(nl)])


@pytest.mark.parametrize("tag", list(SHAPES))
def test_fastcorr_walk_is_exact_on_integers(tag):
    N, nlags, sweeps = _sweeps(tag)
    A = SHAPES[tag][5]
    rng = np.random.default_rng(22 + A)
    s = rng.integers(-1023, 1024, size=N).astype(np.float64)
    met = set()
    for name, info, S, rec in sweeps:
        assert info["A"] == A
        snaps, m = _walk(s, N, info, S, rec)
        met |= m
        assert len(snaps) == len(S)
        # every event position, once where bands share one: the events after a sweep's first run and after its
        # last are among them
        seen = set()
        for S_k, got in snaps:
            if S_k in seen:
                continue
            seen.add(S_k)
            want = _truth(s, N, info["nlo"], info["nhi"], S_k, LANES * A)
            assert np.array_equal(got, want), (tag, name, S_k, int(np.argmax(got != want)))
        print(tag, name, info, "events", len(S), "distinct", len(seen), "blocks in runs", int(rec[:, 0].sum()), sorted(m))
    assert "run" in met or tag in EXTRA, met


def test_cases_occur():
    """Between them the shapes hold a run of one pair and a sweep with no run."""
    met = set()
    for tag in SHAPES:
        for name, info, S, rec in _sweeps(tag)[2]:
            if rec[:, 0].max() == 0:
                met.add("sweep with no run")
            if np.any(rec[:, 0] == 2):
                met.add("run of one pair")
    assert {"sweep with no run", "run of one pair"} <= met, met
