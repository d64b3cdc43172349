"""apply-cmvn | add-deltas | splice-feats (speech_recognition_tools_amd/post.py, csrc/fdlp_post.hip) against the
numpy restatement tests/post_numpy.py.

CPU: the plan's scale tables and sizes, fdlp_cmvn_norm, the restatement's own hand cases, the double-matrix table
reader, the four argparse surfaces.  GPU: bit equality of everything that is a copy or the two-rounding CMVN,
the n-term float32 dot-product bound for the deltas, tile-edge shapes, batch composition, fusion and the CLIs.
Kaldi itself is not available, so parity with its binaries is not pinned here."""
import os
import subprocess

import numpy as np
import pytest

import post_numpy as PN
from conftest import ROOT

BIN = os.path.join(ROOT, "bin")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits_equal(a, b, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(bits(a), bits(b)), what


def ark_like(rng, T, D, shift=0.0):
    """float32 features rounded to 3 decimals like the arks the extractors write"""
    return np.round(rng.standard_normal((T, D)) * 3.0 + shift, 3).astype(np.float32)


def stats_of(x):
    D = x.shape[1]
    st = np.zeros((2, D + 1))
    st[0, :D] = x.astype(np.float64).sum(0)
    st[1, :D] = (x.astype(np.float64) ** 2).sum(0)
    st[0, D] = x.shape[0]
    return st


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_scale_tables_and_out_dim():
    from speech_recognition_tools_amd.post import PostConfig, PostPlan
    p = PostPlan(PostConfig(dim=13, delta_order=2, delta_window=2, left_context=1, right_context=1), device=-1)
    s = p.scales()
    assert p.out_dim == 117 and len(s) == 3
    assert_bits_equal(s[0], np.array([1], dtype=np.float32))
    assert_bits_equal(s[1], np.array([-2, -1, 0, 1, 2], dtype=np.float32) / np.float32(10))
    assert_bits_equal(s[2], np.array([4, 4, 1, -4, -10, -4, 1, 4, 4], dtype=np.float32) / np.float32(100))
    for order, window in ((1, 1), (3, 3), (2, 2), (0, 2)):
        q = PostPlan(PostConfig(dim=7, truncate=5, delta_order=order, delta_window=window, left_context=3), device=-1)
        ref = PN.scale_tables(order, window)
        got = q.scales()
        assert len(got) == order + 1 and q.out_dim == 4 * 5 * (order + 1)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert len(g) == 2 * i * window + 1
            assert_bits_equal(g, r, (order, window, i))


def test_cmvn_norm_hand_cases():
    from speech_recognition_tools_amd._lib import FdlpError
    from speech_recognition_tools_amd.post import cmvn_norm
    # 5 frames; column 0: sum 10, sum of squares 30 (mean 2, var 2); column 1: sum 20, squares 100 (mean 4, var 4)
    st = np.array([[10.0, 20.0, 5.0], [30.0, 100.0, 0.0]])
    assert_bits_equal(cmvn_norm(st), np.array([[1, 1], [-2, -4]], dtype=np.float32))
    r2 = np.sqrt(2.0)
    assert_bits_equal(cmvn_norm(st, norm_vars=True),
                      np.array([[1 / r2, 0.5], [-(2 * (1 / r2)), -2.0]]).astype(np.float32))
    assert_bits_equal(cmvn_norm(st, norm_vars=True, reverse=True), np.array([[r2, 2.0], [2, 4]]).astype(np.float32))
    assert_bits_equal(cmvn_norm(st, reverse=True), np.array([[1, 1], [2, 4]], dtype=np.float32))
    assert_bits_equal(cmvn_norm(st, norm_vars=True, skip_dims=[1]),
                      np.array([[1 / r2, 1.0], [-(2 * (1 / r2)), 0.0]]).astype(np.float32))
    assert_bits_equal(cmvn_norm(st, norm_means=False), np.array([[1, 1], [0, 0]], dtype=np.float32))
    # a constant column: var = 0 is floored at 1e-20, scale = 1e10
    flat = np.array([[15.0, 5.0], [45.0, 0.0]])
    assert_bits_equal(cmvn_norm(flat, norm_vars=True), np.array([[1e10], [-(3.0 * 1e10)]]).astype(np.float32))
    with pytest.raises(FdlpError):
        cmvn_norm(np.array([[1.0, 0.5], [1.0, 0.0]]))            # count < 1
    with pytest.raises(FdlpError, match="variance but not the mean"):
        cmvn_norm(st, norm_means=False, norm_vars=True)
    with pytest.raises(FdlpError):
        cmvn_norm(st, skip_dims=[2])
    # random stats against the restatement
    rng = np.random.default_rng(5)
    x = ark_like(rng, 50, 9, 4.0)
    for kw in (dict(), dict(norm_vars=True), dict(norm_vars=True, reverse=True), dict(norm_vars=True, skip_dims=(0, 8))):
        assert_bits_equal(cmvn_norm(stats_of(x), **kw), PN.cmvn_norm(stats_of(x), **kw), kw)


def test_restatement_hand_cases():
    a, b, T = 0.75, -2.0, 12
    x = (a * np.arange(T) + b).astype(np.float32)[:, None]          # exact in float32
    z, _ = PN.add_deltas(x, 2, 2, dtype=np.float64)
    # t = 0: (-.2 -.1) x0 + .1 x1 + .2 x2 = .5 a;  t = 1: -.2 x0 + .1 (x2 - x0) + .2 x3 = .8 a;  then a
    np.testing.assert_allclose(z[:, 1], [0.5 * a, 0.8 * a] + [a] * (T - 4) + [0.8 * a, 0.5 * a], rtol=1e-6)
    np.testing.assert_allclose(z[4:T - 4, 2], 0.0, atol=1e-6)
    assert np.array_equal(z[:, 0], x[:, 0])
    one = np.array([[1.5, -2.25, 3.0]], dtype=np.float32)
    # T = 1: every tap sees the one row and the taps sum to zero, so the deltas vanish up to the rounding of the
    # float32 sum (the dot-product bound of the GPU test); the splice repeats the row
    z1, mag = PN.add_deltas(one, 2, 2)
    assert np.array_equal(z1[:, :3], one)
    assert np.all(np.abs(z1[:, 3:]) <= 11 * 2.0 ** -24 * mag[:, 3:])
    z1d, _ = PN.add_deltas(one, 2, 2, dtype=np.float64)
    np.testing.assert_allclose(z1d[:, 3:], 0.0, atol=1e-7)
    assert np.array_equal(PN.splice(z1, 2, 1), np.tile(z1, (1, 4)))
    y = np.arange(8, dtype=np.float32).reshape(4, 2)
    assert np.array_equal(PN.splice(y, 1, 1)[0], [0, 1, 0, 1, 2, 3])
    assert np.array_equal(PN.splice(y, 1, 1)[3], [4, 5, 6, 7, 6, 7])
    assert np.array_equal(PN.add_deltas(y, 0, 2, truncate=1)[0], y[:, :1])


def test_double_matrix_table_round_trip(tmp_path):
    from speech_recognition_tools_amd.cmvn import write_table
    from speech_recognition_tools_amd.post import read_dmatrix_table
    rng = np.random.default_rng(2)
    # values that do not survive float32
    items = [("spk%d" % i, rng.standard_normal((2, 6)) * 1e9 + 0.123456789) for i in range(3)]
    ark, scp = str(tmp_path / "s.ark"), str(tmp_path / "s.scp")
    write_table("ark,scp:%s,%s" % (ark, scp), items)
    for spec in ("ark:" + ark, "scp:" + scp, "ark,s,cs:" + ark, "scp,p:" + scp):
        got = list(read_dmatrix_table(spec))
        assert [k for k, _ in got] == [k for k, _ in items]
        for (_, g), (_, m) in zip(got, items):
            assert g.dtype == np.float64 and np.array_equal(g, m)


def test_cli_argparse_surfaces():
    from speech_recognition_tools_amd import post
    a = post.apply_cmvn_parser().parse_args(["cmvn.ark", "scp:f.scp", "ark:-"])
    assert (a.norm_means, a.norm_vars, a.reverse, a.skip_dims, a.utt2spk) == (True, False, False, (), "")
    assert (a.cmvn, a.feats, a.out) == ("cmvn.ark", "scp:f.scp", "ark:-")
    a = post.apply_cmvn_parser().parse_args(["--norm-vars=true", "--norm-means=false", "--reverse=true",
                                             "--skip-dims=0:3:12", "--utt2spk=ark:u2s", "ark:c", "ark:i", "ark:o"])
    assert (a.norm_means, a.norm_vars, a.reverse, a.skip_dims, a.utt2spk) == (False, True, True, (0, 3, 12), "ark:u2s")
    a = post.add_deltas_parser().parse_args(["ark:i", "ark:o"])
    assert (a.delta_order, a.delta_window, a.truncate) == (2, 2, 0)
    a = post.add_deltas_parser().parse_args(["--delta-order=3", "--delta-window=1", "--truncate=5", "ark:i", "ark:o"])
    assert (a.delta_order, a.delta_window, a.truncate) == (3, 1, 5)
    a = post.splice_feats_parser().parse_args(["ark:i", "ark:o"])
    assert (a.left_context, a.right_context) == (4, 4)
    a = post.splice_feats_parser().parse_args(["--left-context=3", "--right-context=0", "ark:i", "ark:o"])
    assert (a.left_context, a.right_context) == (3, 0)
    a = post.post_feats_parser().parse_args(["--cmvn=ark:c", "--utt2spk=ark:u", "--norm-vars=true", "--delta-order=2",
                                             "--left-context=4", "--right-context=4", "scp:i", "ark,scp:o.ark,o.scp"])
    assert (a.cmvn, a.utt2spk, a.norm_vars, a.delta_order, a.delta_window, a.truncate, a.left_context,
            a.right_context) == ("ark:c", "ark:u", True, 2, 2, 0, 4, 4)
    a = post.post_feats_parser().parse_args(["scp:i", "ark:o"])   # every stage off
    assert (a.cmvn, a.norm_means, a.norm_vars, a.delta_order, a.left_context, a.right_context) == ("", True, False, 0, 0, 0)
    for name in post.MAINS:
        assert os.access(os.path.join(BIN, name), os.X_OK), name


def test_host_plan_tiles_and_capacity_refusal():
    from speech_recognition_tools_amd._lib import FDLP_E_INVALID, FdlpError
    from speech_recognition_tools_amd.post import PostConfig, PostPlan
    with pytest.raises(FdlpError) as e:
        PostPlan(PostConfig(dim=4096, left_context=20, right_context=20), device=-1)
    assert e.value.code == FDLP_E_INVALID
    assert "4096" in str(e.value) and "20" in str(e.value) and str(4096 * 41) in str(e.value)
    for D in (13, 80, 440):
        p = PostPlan(PostConfig(dim=D, delta_order=2, delta_window=2, left_context=4, right_context=4), device=-1)
        assert p.out_dim == 27 * D and p.tile >= 1 and 0 < p.lds_bytes <= 160 * 1024
        # the reported LDS bytes are the two tiles of the documented shape
        a = (p.tile + 8 + 8) * D
        assert p.lds_bytes == 4 * ((a + 3) // 4 * 4 + (p.tile + 8) * 3 * D)
    with pytest.raises(FdlpError):
        PostPlan(PostConfig(dim=13, truncate=14), device=-1)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def check_utterance(g, x, norm, norm_vars, order, window, truncate, L, R):
    """g: the device rows [T, Dout] of one utterance with input x."""
    D = truncate or x.shape[1]
    Dp = D * (order + 1)
    assert g.shape == (x.shape[0], Dp * (L + R + 1))
    z = g[:, L * Dp:(L + 1) * Dp]                           # the frame's own delta-augmented row
    assert_bits_equal(g, PN.splice(z, L, R), "splice copies")
    y = PN.apply_cmvn(x, norm, norm_vars)
    assert_bits_equal(z[:, :D], y[:, :D], "cmvn / order-0 columns")
    if order:
        r, mag = PN.add_deltas(y, order, window, truncate, dtype=np.float64)
        n = 2 * order * window + 1
        err = np.abs(z.astype(np.float64) - r)[:, D:]
        bound = ((n + 2) * 2.0 ** -24 * mag)[:, D:]
        assert np.all(err <= bound), (float((err - bound).max()), float(err.max()))


def run_batch(plan, xs, norms=None, idx=None, norm_vars=True, out=None):
    import torch
    feats = torch.from_numpy(np.concatenate(xs)).cuda()
    nt = torch.from_numpy(np.stack(norms)).cuda() if norms is not None else None
    o = plan.compute(feats, [x.shape[0] for x in xs], norm=nt, norm_index=idx, norm_vars=norm_vars, out=out)
    torch.cuda.synchronize()
    return o.cpu().numpy()


def split_rows(a, xs):
    ends = np.cumsum([x.shape[0] for x in xs])
    return [a[e - x.shape[0]:e] for e, x in zip(ends, xs)]


# D, order, window, L, R, truncate: every D of {1, 13, 80}, every (order, window) of {(0,2), (1,1), (2,2), (3,3)},
# every (L, R) of {(0,0), (3,0), (0,2), (4,4)}, truncate 5 of 13; (13, 2, 2, 1, 1) has 117-column rows
SHAPES = [(1, 0, 2, 0, 0, 0), (1, 2, 2, 4, 4, 0), (1, 3, 3, 3, 0, 0), (13, 2, 2, 1, 1, 0), (13, 1, 1, 3, 0, 5),
          (13, 3, 3, 0, 2, 0), (13, 0, 2, 4, 4, 0), (80, 2, 2, 4, 4, 0), (80, 0, 2, 3, 0, 0), (80, 1, 1, 0, 0, 0),
          (80, 0, 2, 0, 0, 0), (80, 3, 3, 0, 2, 0),
          (13, 1, 2, 0, 0, 0), (80, 3, 2, 1, 1, 0)]  # window 2: the order-1 kernel, and order 3 on the general one
# rows too wide for 16 frames per tile: shape -> (tile, LDS bytes) of the plain chain.  One frame per tile above 64 KB
# (the launch raises the kernel's dynamic LDS limit first) in each of post_kernel's four code objects, and tiles 2, 4, 8
SMALL_TILES = {(440, 2, 2, 4, 4, 0): (1, 77440), (600, 0, 2, 16, 15, 0): (1, 76800), (450, 1, 1, 10, 10, 0): (1, 117008),
               (350, 1, 2, 8, 8, 0): (1, 77008), (400, 2, 2, 3, 3, 0): (2, 64000), (333, 1, 2, 5, 4, 0): (4, 57288),
               (120, 2, 2, 10, 10, 0): (8, 57600)}
SHAPES += list(SMALL_TILES)


def test_small_tile_shapes_have_their_tiles():
    from speech_recognition_tools_amd.post import PostConfig, PostPlan
    for (D, order, window, L, R, truncate), want in SMALL_TILES.items():
        p = PostPlan(PostConfig(dim=D, truncate=truncate, delta_order=order, delta_window=window, left_context=L,
                                right_context=R), device=-1)
        assert (p.tile, p.lds_bytes) == want, (D, order, window, L, R)
    assert sorted(t for t, _ in SMALL_TILES.values()) == [1, 1, 1, 1, 2, 4, 8]
    assert sum(b > 65536 for _, b in SMALL_TILES.values()) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("D,order,window,L,R,truncate", SHAPES)
def test_gpu_exact_over_shapes(D, order, window, L, R, truncate):
    from speech_recognition_tools_amd.post import PostConfig, PostPlan
    plan = PostPlan(PostConfig(dim=D, truncate=truncate, delta_order=order, delta_window=window, left_context=L,
                               right_context=R))
    TF = plan.tile
    halo = max(L, R) + order * window
    Ts = sorted({T for T in (1, 2, 3, halo - 1, halo, TF - 1, TF, TF + 1, 2 * TF + 3) if T >= 1})
    rng = np.random.default_rng(D * 1000 + order * 100 + L * 10 + R)
    xs = [ark_like(rng, T, D, 2.0 * (i % 2)) for i, T in enumerate(Ts)]
    norms = [PN.cmvn_norm(stats_of(np.concatenate(xs[k::2])), norm_vars=True) for k in (0, 1)]
    idx = [i % 2 for i in range(len(xs))]
    got = run_batch(plan, xs, norms, idx)
    for g, x, k in zip(split_rows(got, xs), xs, idx):
        check_utterance(g, x, norms[k], True, order, window, truncate, L, R)
    # means only (no multiply) and no CMVN at all
    mo = PN.cmvn_norm(stats_of(np.concatenate(xs)))
    for g, x in zip(split_rows(run_batch(plan, xs, [mo], None, norm_vars=False), xs), xs):
        check_utterance(g, x, mo, False, order, window, truncate, L, R)
    for g, x in zip(split_rows(run_batch(plan, xs), xs), xs):
        check_utterance(g, x, None, False, order, window, truncate, L, R)


@pytest.fixture(scope="module")
def batch40():
    """~40 utterances of 13 columns with runs of adjacent 1-frame utterances, two speakers interleaved"""
    rng = np.random.default_rng(40)
    Ts = [1, 1, 1, 7, 1, 300, 2, 1, 1, 129, 128, 127, 3, 1] + [int(t) for t in rng.integers(1, 200, 22)] + [1, 1, 1, 64]
    xs = [ark_like(rng, T, 13, 1.5 * (i % 2)) for i, T in enumerate(Ts)]
    norms = [PN.cmvn_norm(stats_of(np.concatenate(xs[k::2])), norm_vars=True) for k in (0, 1)]
    idx = [i % 2 for i in range(len(xs))]
    return xs, norms, idx


@pytest.mark.gpu
def test_gpu_batch_composition(batch40):
    import torch
    from speech_recognition_tools_amd.post import PostConfig, PostPlan
    xs, norms, idx = batch40
    plan = PostPlan(PostConfig(dim=13, delta_order=2, delta_window=2, left_context=1, right_context=1))
    rows = sum(x.shape[0] for x in xs)
    SENT = np.float32(-12345.5)
    out = torch.full((rows + 5, plan.out_dim), float(SENT), dtype=torch.float32, device="cuda")
    got = run_batch(plan, xs, norms, idx, out=out)
    assert np.all(got[rows:] == SENT), "rows after the output were written"
    got = got[:rows]
    for g, x, k in zip(split_rows(got, xs), xs, idx):
        check_utterance(g, x, norms[k], True, 2, 2, 0, 1, 1)
    # one utterance per call
    for g, x, k in zip(split_rows(got, xs), xs, idx):
        assert_bits_equal(run_batch(plan, [x], [norms[k]], None), g, "one per call")
    # every other utterance NaN: the others stay finite and unchanged
    xn = [np.full_like(x, np.nan) if i % 2 else x for i, x in enumerate(xs)]
    gn = run_batch(plan, xn, norms, idx)
    for i, (a, b) in enumerate(zip(split_rows(gn, xs), split_rows(got, xs))):
        if i % 2:
            assert np.all(np.isnan(a))
        else:
            assert np.all(np.isfinite(a))
            assert_bits_equal(a, b, "neighbour of a NaN utterance")


@pytest.mark.gpu
def test_gpu_fused_equals_chained():
    import torch
    from speech_recognition_tools_amd.post import PostConfig, PostPlan
    rng = np.random.default_rng(3)
    for D, order, window, L, R, truncate in ((13, 2, 2, 1, 1, 0), (80, 2, 2, 4, 4, 0), (13, 3, 3, 3, 0, 5)):
        xs = [ark_like(rng, T, D, 1.0) for T in (1, 2, 40, 131, 5)]
        lens = [x.shape[0] for x in xs]
        norm = torch.from_numpy(PN.cmvn_norm(stats_of(np.concatenate(xs)), norm_vars=True)).cuda()
        feats = torch.from_numpy(np.concatenate(xs)).cuda()
        fused = PostPlan(PostConfig(dim=D, truncate=truncate, delta_order=order, delta_window=window, left_context=L,
                                    right_context=R)).compute(feats, lens, norm=norm)
        a = PostPlan(PostConfig(dim=D)).compute(feats, lens, norm=norm)
        b = PostPlan(PostConfig(dim=D, truncate=truncate, delta_order=order, delta_window=window)).compute(a, lens)
        c = PostPlan(PostConfig(dim=b.shape[1], left_context=L, right_context=R)).compute(b, lens)
        torch.cuda.synchronize()
        assert_bits_equal(fused.cpu().numpy(), c.cpu().numpy(), (D, order, L, R))


CHECKS_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import torch
import test_post as TP
from speech_recognition_tools_amd.plan import device_checks
from speech_recognition_tools_amd.post import PostConfig, PostPlan
assert device_checks(reset=True)[0], "not a checks build"
rng = np.random.default_rng(1)
runs = 0
for D, order, window, L, R, truncate in TP.SHAPES:
    plan = PostPlan(PostConfig(dim=D, truncate=truncate, delta_order=order, delta_window=window, left_context=L,
                               right_context=R))
    TF = plan.tile
    xs = [TP.ark_like(rng, T, D) for T in (1, 1, 2, TF - 1, TF, TF + 1, 2 * TF + 3, 1) if T >= 1]
    norm = [TP.PN.cmvn_norm(TP.stats_of(np.concatenate(xs)), norm_vars=True)]
    # an output that starts 4, 8 and 12 bytes past a 16-byte boundary as well
    for shift in range(4):
        rows = sum(x.shape[0] for x in xs)
        flat = torch.empty(rows * plan.out_dim + 4, dtype=torch.float32, device="cuda")
        out = flat[shift:shift + rows * plan.out_dim].view(rows, plan.out_dim)
        got = TP.run_batch(plan, xs, norm, None, out=out)
        if shift == 0:
            first = got
        assert np.array_equal(TP.bits(got), TP.bits(first))
        runs += 1
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": runs}))
"""


@pytest.mark.gpu
def test_gpu_device_range_checks_silent():
    """the FDLP_DEVICE_CHECKS build of post_kernel over every shape, with outputs at all four 4-byte phases"""
    import json
    import sys
    lib = os.path.join(ROOT, "speech_recognition_tools_amd", "lib", "libfdlp_checks.so")
    assert os.path.exists(lib), "build() compiles libfdlp_checks.so"
    r = subprocess.run([sys.executable, "-c", CHECKS_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=dict(os.environ, FDLP_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["enabled"] and res["runs"] == 4 * len(SHAPES)
    assert res["violations"] == 0, res


def _write_ark(path, items, scp=None):
    from speech_recognition_tools_amd.post import FeatWriter
    w = FeatWriter("ark,scp:%s,%s" % (path, scp) if scp else "ark:" + path)
    for k, m in items:
        w.write(k, m)
    w.close()


@pytest.mark.gpu
def test_gpu_cli_chain_pipe_and_errors(tmp_path):
    from speech_recognition_tools_amd import cmvn, post
    from speech_recognition_tools_amd.cmvn import MatReader
    rng = np.random.default_rng(11)
    utts = [("s%d_u%d" % (i % 2, i), ark_like(rng, T, 13, float(i % 2))) for i, T in enumerate((5, 1, 90, 33, 1, 140))]
    utts.append(("s9_u0", ark_like(rng, 4, 13)))            # a speaker without stats
    d = str(tmp_path)
    feats, scp = d + "/feats.ark", d + "/feats.scp"
    _write_ark(feats, utts, scp)
    with open(d + "/utt2spk", "w") as f:
        f.writelines("%s %s\n" % (k, k.split("_")[0]) for k, _ in utts)
    with open(d + "/spk2utt", "w") as f:
        for s in ("s0", "s1"):
            f.write(s + " " + " ".join(k for k, _ in utts if k.startswith(s + "_")) + "\n")
    assert cmvn.main(["--spk2utt=ark:" + d + "/spk2utt", "scp:" + scp, "ark:" + d + "/cmvn.ark"]) == 0
    copts = ["--norm-vars=true", "--utt2spk=ark:" + d + "/utt2spk"]
    assert post.main_post_feats(copts + ["--cmvn=ark:" + d + "/cmvn.ark", "--delta-order=2", "--left-context=3",
                                         "--right-context=2", "scp:" + scp, "ark,scp:%s/fused.ark,%s/fused.scp" % (d, d)]) == 0
    assert post.main_apply_cmvn(copts + ["ark:" + d + "/cmvn.ark", "scp:" + scp, "ark:" + d + "/a.ark"]) == 0
    assert post.main_add_deltas(["ark:" + d + "/a.ark", "ark:" + d + "/b.ark"]) == 0
    assert post.main_splice_feats(["--left-context=3", "--right-context=2", "ark,s,cs:" + d + "/b.ark",
                                   "ark:" + d + "/c.ark"]) == 0
    fused = open(d + "/fused.ark", "rb").read()
    assert fused == open(d + "/c.ark", "rb").read()
    # the utterance without stats is skipped, and the rows are the restatement's
    got = dict((k, m.copy()) for k, m in MatReader("scp:" + d + "/fused.scp"))
    assert list(got) == [k for k, _ in utts[:-1]]
    stats = dict(post.read_dmatrix_table("ark:" + d + "/cmvn.ark"))
    for k, x in utts[:-1]:
        check_utterance(got[k], x, PN.cmvn_norm(stats[k.split("_")[0]], norm_vars=True), True, 2, 2, 0, 3, 2)
    # one ark:- pipe of two drop-ins, as the recipes compose them; the skipped utterance is counted
    env = dict(os.environ)
    cmd = ("set -o pipefail; %s/apply-cmvn %s ark:%s/cmvn.ark scp:%s ark:- 2>%s/e1 | %s/add-deltas ark:- ark:%s/b2.ark 2>%s/e2"
           % (BIN, " ".join(copts), d, scp, d, BIN, d, d))
    r = subprocess.run(["bash", "-c", cmd], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, open(d + "/e1").read()[-2000:] + open(d + "/e2").read()[-2000:]
    assert open(d + "/b2.ark", "rb").read() == open(d + "/b.ark", "rb").read()
    e1 = open(d + "/e1").read()
    assert "No normalization statistics available for key s9_u0" in e1
    assert "Applied cepstral mean and variance normalization to 6 utterances, errors on 1" in e1
    # empty input: exit status 1
    open(d + "/empty.scp", "w").close()
    r = subprocess.run([BIN + "/splice-feats", "scp:" + d + "/empty.scp", "ark:" + d + "/none.ark"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stderr[-2000:]
    assert "to 0 utterances" in r.stderr
    assert not [f for f in os.listdir(d) if f.endswith(".tmp")]
