"""transform-feats fused after the splice (speech_recognition_tools_amd/post.py XformPlan, xform_kernel of
csrc/fdlp_post.hip): out = A M[:, :K]^T (+ M[:, K]) on the float32 MFMA, A being the rows the other stages give.

The reference is the float64 product of the float32 rows entering the transform (the plain PostPlan's output,
which tests/test_post.py holds to the numpy restatement) with the float32 matrix.  A float32 dot product of K
terms in any order plus one add satisfies, elementwise and for K <= 4096,

    |got - ref| <= (K + 2) 2^-24 (|A| |M[:, :K]|^T + |M[:, K]|)

(the gamma_K bound, the form test_post.py uses for the deltas); that is asserted as it stands.  Everything that
is a claim of independence (batch composition, tile position, fused against chained) is asserted bitwise.
Kaldi itself is not available, so parity with its binary is not pinned here."""
import os
import struct
import subprocess

import numpy as np
import pytest

import post_numpy as PN
from conftest import ROOT

BIN = os.path.join(ROOT, "bin")
KC = 32   # columns k of the matrix staged in LDS at a time (kXfKC)


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


def make_mat(rng, N, K, affine):
    """seeded normal scaled by 1/sqrt(K); the offset column (affine) of order one"""
    m = rng.standard_normal((N, K + int(affine))) / np.sqrt(K)
    if affine:
        m[:, K] = rng.standard_normal(N)
    return m.astype(np.float32)


def ref_and_bound(A, M):
    """float64 reference and the elementwise bound of the module docstring for float32 rows A and matrix M"""
    K = A.shape[1]
    assert K <= 4096 and M.shape[1] in (K, K + 1)
    A64, M64 = A.astype(np.float64), M.astype(np.float64)
    ref = A64 @ M64[:, :K].T
    mag = np.abs(A64) @ np.abs(M64[:, :K]).T
    if M.shape[1] == K + 1:
        ref = ref + M64[:, K]
        mag = mag + np.abs(M64[:, K])
    return ref, (K + 2) * 2.0 ** -24 * mag


def assert_within_bound(got, A, M, what=""):
    ref, bound = ref_and_bound(A, M)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    print("%s: max err %.3g, max err/bound %.3g" % (what, float(err.max()), float((err / bound).max())))
    assert np.all(err <= bound), (what, float((err - bound).max()), float(err.max()))


def write_fm(path, m):
    m = np.ascontiguousarray(m, dtype="<f4")
    with open(path, "wb") as f:
        f.write(b"\0BFM \x04" + struct.pack("<i", m.shape[0]) + b"\x04" + struct.pack("<i", m.shape[1]) + m.tobytes())


def write_dm(path, m):
    m = np.ascontiguousarray(m, dtype="<f8")
    with open(path, "wb") as f:
        f.write(b"\0BDM \x04" + struct.pack("<i", m.shape[0]) + b"\x04" + struct.pack("<i", m.shape[1]) + m.tobytes())


def write_text(path, m):
    with open(path, "w") as f:
        f.write(" [\n" + "\n".join("  " + " ".join(repr(float(v)) for v in r) for r in m) + " ]\n")


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_cli_argparse_surfaces():
    from speech_recognition_tools_amd import post
    a = post.transform_feats_parser().parse_args(["final.mat", "ark:-", "ark:-"])
    assert (a.utt2spk, a.transform, a.feats, a.out, a.batch_rows) == ("", "final.mat", "ark:-", "ark:-", 16384)
    a = post.transform_feats_parser().parse_args(["--utt2spk=ark:u2s", "--device=1", "--batch-rows=512", "ark:t.ark",
                                                  "scp:f.scp", "ark,scp:o.ark,o.scp"])
    assert (a.utt2spk, a.device, a.batch_rows, a.transform, a.feats, a.out) == (
        "ark:u2s", 1, 512, "ark:t.ark", "scp:f.scp", "ark,scp:o.ark,o.scp")
    a = post.post_feats_parser().parse_args(["scp:i", "ark:o"])
    assert a.transform == ""                                   # the stage is off by default
    a = post.post_feats_parser().parse_args(["--norm-vars=true", "--utt2spk=ark:u", "--cmvn=scp:c.scp",
                                             "--left-context=4", "--right-context=4", "--transform=exp/final.mat",
                                             "scp:i", "ark:-"])
    assert (a.transform, a.cmvn, a.utt2spk, a.left_context, a.right_context) == ("exp/final.mat", "scp:c.scp", "ark:u", 4, 4)
    assert post.MAINS["transform-feats"] is post.main_transform_feats
    assert os.access(os.path.join(BIN, "transform-feats"), os.X_OK)


def test_matrix_file_reader(tmp_path):
    from speech_recognition_tools_amd.cmvn import read_kaldi_dmatrix
    from speech_recognition_tools_amd.post import read_kaldi_matrix
    rng = np.random.default_rng(8)
    m = rng.standard_normal((5, 7)) * 1e3 + 0.123456789      # does not survive float32
    f32 = m.astype(np.float32)
    p = str(tmp_path / "m")
    write_fm(p, f32)
    got = read_kaldi_matrix(p)
    assert got.dtype == np.float32
    assert_bits_equal(got, f32, "FM")
    with pytest.raises(ValueError):
        read_kaldi_dmatrix(p)                                 # the stats reader still refuses a float matrix
    write_dm(p, m)
    assert_bits_equal(read_kaldi_matrix(p), f32, "DM is rounded once")
    write_text(p, m)
    assert_bits_equal(read_kaldi_matrix(p), f32, "text")
    write_text(p, m[:1])
    assert read_kaldi_matrix(p).shape == (1, 7)
    # truncated files are refused in every form
    write_fm(p, f32)
    raw = open(p, "rb").read()
    for cut in (len(raw) - 1, 20, 14, 9):
        open(p, "wb").write(raw[:cut])
        with pytest.raises(ValueError):
            read_kaldi_matrix(p)
    write_dm(p, m)
    open(p, "wb").write(open(p, "rb").read()[:-8])
    with pytest.raises(ValueError):
        read_kaldi_matrix(p)
    write_text(p, m)
    open(p, "w").write(open(p).read().rstrip()[:-1])          # the closing bracket is missing
    with pytest.raises(ValueError):
        read_kaldi_matrix(p)
    open(p, "w").write(" [\n 1 2 3\n 4 5 ]\n")
    with pytest.raises(ValueError):
        read_kaldi_matrix(p)
    open(p, "wb").write(b"\0BCM \x04")
    with pytest.raises(ValueError):
        read_kaldi_matrix(p)


def chunk_floats(N):
    ncb = min((N + 15) // 16, 4)
    return 2 * KC * (16 * ncb + 4)                           # two buffers of KC rows, 4 floats of padding each


@pytest.mark.parametrize("D,order,L,R,N,affine", [(13, 2, 4, 4, 40, True), (80, 0, 4, 4, 40, False)])
def test_host_plan_info(D, order, L, R, N, affine):
    from speech_recognition_tools_amd.post import PostConfig, XformPlan
    p = XformPlan(PostConfig(dim=D, delta_order=order, delta_window=2, left_context=L, right_context=R), N, affine,
                  device=-1)
    K = D * (order + 1) * (L + R + 1)
    assert (p.in_dim, p.out_dim, p.mat_cols) == (K, N, K + int(affine))
    assert p.tile >= 16 and p.tile & (p.tile - 1) == 0
    a = (p.tile + L + R + 4 * order) * D if order else 0
    want = 4 * ((a + 3) // 4 * 4 + (p.tile + L + R) * D * (order + 1) + chunk_floats(N))
    assert p.lds_bytes == want and want <= 64 * 1024
    assert chunk_floats(40) == 2 * 32 * 52


def test_capacity_and_argument_refusals():
    from speech_recognition_tools_amd._lib import FDLP_E_INVALID, FdlpError
    from speech_recognition_tools_amd.post import PostConfig, XformPlan
    with pytest.raises(FdlpError) as e:
        XformPlan(PostConfig(dim=4096, left_context=20, right_context=20), 40, device=-1)
    assert e.value.code == FDLP_E_INVALID
    assert "4096" in str(e.value) and str(4096 * 41) in str(e.value) and "40 columns" in str(e.value)
    # the chunk of the matrix is what no longer fits: the plain chain takes 40000 columns at one frame per tile
    from speech_recognition_tools_amd.post import PostPlan
    assert PostPlan(PostConfig(dim=40000), device=-1).tile == 1
    with pytest.raises(FdlpError) as e:
        XformPlan(PostConfig(dim=40000), 40, device=-1)
    assert e.value.code == FDLP_E_INVALID and "40000" in str(e.value)
    for n in (0, -3, 65537):
        with pytest.raises(FdlpError) as e:
            XformPlan(PostConfig(dim=13), n, device=-1)
        assert e.value.code == FDLP_E_INVALID and str(n) in str(e.value)
    with pytest.raises(FdlpError):
        XformPlan(PostConfig(dim=13, truncate=14), 13, device=-1)
    with pytest.raises(FdlpError):
        XformPlan(PostConfig(dim=13, delta_order=9), 13, device=-1)
    assert XformPlan(PostConfig(dim=13), 65536, device=-1).out_dim == 65536


def test_new_entry_points_are_declared_and_exported():
    import re
    from speech_recognition_tools_amd import _lib
    names = ["fdlp_xform_plan_create", "fdlp_xform_plan_destroy", "fdlp_xform_plan_info", "fdlp_xform_plan_dispatch",
             "fdlp_xform_compute"]
    src = open(os.path.join(ROOT, "include", "fdlp.h")).read()
    declared = set(re.findall(r"\b(fdlp_[a-z0-9_]+)\s*\(", src))
    for n in names:
        assert n in declared and n in _lib.SIGNATURES and hasattr(_lib.lib, n), n
    assert sorted(n for n in _lib.SIGNATURES if "xform" in n) == sorted(names)
    assert "#define FDLP_ABI_VERSION 13" in src and _lib.lib.fdlp_abi_version() == 13
    # a host-only plan refuses to compute, and null arguments are refused
    import ctypes
    from speech_recognition_tools_amd._lib import FdlpError, FdlpPostBatchC, check
    from speech_recognition_tools_amd.post import PostConfig, XformPlan
    p = XformPlan(PostConfig(dim=13), 13, True, device=-1)
    with pytest.raises(FdlpError):
        check(_lib.lib.fdlp_xform_compute(p._h, ctypes.byref(FdlpPostBatchC()), None, 1, None, None))
    with pytest.raises(FdlpError):
        check(_lib.lib.fdlp_xform_plan_info(None, None, None, None, None, None))


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def run_xform(plan, xs, mats, midx=None, norms=None, idx=None, out=None):
    import torch
    feats = torch.from_numpy(np.concatenate(xs)).cuda()
    nt = torch.from_numpy(np.stack(norms)).cuda() if norms is not None else None
    mt = torch.from_numpy(np.stack(mats)).cuda()
    o = plan.compute(feats, [x.shape[0] for x in xs], mt, midx, norm=nt, norm_index=idx, out=out)
    torch.cuda.synchronize()
    return o.cpu().numpy()


def run_post(plan, xs, norms=None, idx=None):
    import torch
    feats = torch.from_numpy(np.concatenate(xs)).cuda()
    nt = torch.from_numpy(np.stack(norms)).cuda() if norms is not None else None
    o = plan.compute(feats, [x.shape[0] for x in xs], norm=nt, norm_index=idx)
    torch.cuda.synchronize()
    return o.cpu().numpy()


def split_rows(a, xs):
    ends = np.cumsum([x.shape[0] for x in xs])
    return [a[e - x.shape[0]:e] for e, x in zip(ends, xs)]


# D, order, window, L, R, N, affine
SHAPES = [(1, 0, 2, 0, 0, 1, False),      # K = 1
          (13, 0, 2, 4, 4, 40, False),    # K = 117: K mod 4 = 1, N mod 16 = 8
          (13, 2, 2, 4, 4, 40, True),     # K = 351
          (80, 0, 2, 4, 4, 40, True),     # K = 720
          (80, 2, 2, 4, 4, 17, False),    # K = 2160
          (13, 0, 2, 0, 0, 13, True),     # a stand-alone fMLLR shape
          (5, 1, 1, 3, 0, 48, False)]


def shape_case(D, order, window, L, R, N, affine, tile, seed):
    rng = np.random.default_rng(seed)
    Ts = [T for T in (1, 2, 3, 15, 16, 17, 33, tile - 1, tile, tile + 1, 2 * tile + 3) if T >= 1]
    xs = [ark_like(rng, T, D, 2.0 * (i % 2)) for i, T in enumerate(Ts)]
    norms = [PN.cmvn_norm(stats_of(np.concatenate(xs[k::2])), norm_vars=True) for k in (0, 1)]
    idx = [i % 2 for i in range(len(xs))]
    K = D * (order + 1) * (L + R + 1)
    mats = [make_mat(rng, N, K, affine) for _ in range(2)]
    midx = [(i // 2) % 2 for i in range(len(xs))]           # not in step with the norm index
    return xs, norms, idx, mats, midx


@pytest.mark.gpu
@pytest.mark.parametrize("D,order,window,L,R,N,affine", SHAPES)
def test_gpu_bound_over_shapes(D, order, window, L, R, N, affine):
    from speech_recognition_tools_amd.post import PostConfig, PostPlan, XformPlan
    cfg = PostConfig(dim=D, delta_order=order, delta_window=window, left_context=L, right_context=R)
    plan = XformPlan(cfg, N, affine)
    xs, norms, idx, mats, midx = shape_case(D, order, window, L, R, N, affine, plan.tile, D * 1000 + N)
    K = plan.in_dim
    assert K == D * (order + 1) * (L + R + 1) and plan.mat_cols == K + int(affine)
    got = run_xform(plan, xs, mats, midx, norms, idx)
    assert got.shape == (sum(x.shape[0] for x in xs), N)
    rows = run_post(PostPlan(cfg), xs, norms, idx)          # the float32 rows entering the transform
    for i, (g, A, x) in enumerate(zip(split_rows(got, xs), split_rows(rows, xs), xs)):
        if order == 0:
            assert_bits_equal(A, PN.post(x, norms[idx[i]], True, 0, window, 0, L, R), "rows entering the transform")
        assert_within_bound(g, A, mats[midx[i]], "K %d N %d T %d" % (K, N, x.shape[0]))
    # NULL mat_index is matrix 0 for every utterance; no CMVN at all
    got0 = run_xform(plan, xs, mats)
    rows0 = run_post(PostPlan(cfg), xs)
    for g, A in zip(split_rows(got0, xs), split_rows(rows0, xs)):
        assert_within_bound(g, A, mats[0], "matrix 0, no cmvn")


@pytest.fixture(scope="module")
def batch40():
    """~40 utterances of 13 columns with runs of adjacent 1-frame utterances, two speakers interleaved"""
    rng = np.random.default_rng(40)
    Ts = [1, 1, 1, 7, 1, 300, 2, 1, 1, 129, 128, 127, 3, 1] + [int(t) for t in rng.integers(1, 200, 22)] + [1, 1, 1, 64]
    xs = [ark_like(rng, T, 13, 1.5 * (i % 2)) for i, T in enumerate(Ts)]
    norms = [PN.cmvn_norm(stats_of(np.concatenate(xs[k::2])), norm_vars=True) for k in (0, 1)]
    idx = [i % 2 for i in range(len(xs))]
    mats = [make_mat(rng, 40, 351, True) for _ in range(2)]
    return xs, norms, idx, mats


@pytest.mark.gpu
def test_gpu_batch_composition(batch40):
    import torch
    from speech_recognition_tools_amd.post import PostConfig, PostPlan, XformPlan
    xs, norms, idx, mats = batch40
    cfg = PostConfig(dim=13, delta_order=2, delta_window=2, left_context=4, right_context=4)
    plan = XformPlan(cfg, 40, True)
    # the NaN batch runs first, so that NaNs are what a later workgroup finds in the LDS
    xn = [np.full_like(x, np.nan) if i % 2 else x for i, x in enumerate(xs)]
    gn = run_xform(plan, xn, mats, idx, norms, idx)
    rows = sum(x.shape[0] for x in xs)
    SENT = np.float32(-12345.5)
    out = torch.full((rows + 5, 40), float(SENT), dtype=torch.float32, device="cuda")
    got = run_xform(plan, xs, mats, idx, norms, idx, out=out)
    assert np.all(got[rows:] == SENT), "rows after the output were written"
    got = got[:rows]
    A = run_post(PostPlan(cfg), xs, norms, idx)
    for g, a, k in zip(split_rows(got, xs), split_rows(A, xs), idx):
        assert_within_bound(g, a, mats[k], "batch40")
    for i, (a, b) in enumerate(zip(split_rows(gn, xs), split_rows(got, xs))):
        if i % 2:
            assert np.all(np.isnan(a))
        else:
            assert np.all(np.isfinite(a))
            assert_bits_equal(a, b, "neighbour of a NaN utterance")
    # one utterance per call: bitwise the rows it has in the batch
    for g, x, k in zip(split_rows(got, xs), xs, idx):
        assert_bits_equal(run_xform(plan, [x], [mats[k]], None, [norms[k]], None), g, "one per call")
    # and at other tile positions: the utterance after a prefix of another length
    g300 = split_rows(got, xs)[5]
    for pre in (1, 17):
        both = run_xform(plan, [xs[9][:pre], xs[5]], mats, [0, idx[5]], norms, [0, idx[5]])
        assert_bits_equal(both[pre:], g300, "after a prefix of %d rows" % pre)


@pytest.mark.gpu
def test_gpu_fused_equals_chained():
    import torch
    from speech_recognition_tools_amd.post import PostConfig, PostPlan, XformPlan
    rng = np.random.default_rng(3)
    for D, order, window, L, R, N, affine in ((13, 2, 2, 4, 4, 40, True), (80, 0, 2, 4, 4, 40, False),
                                              (5, 1, 1, 3, 0, 48, False)):
        xs = [ark_like(rng, T, D, 1.0) for T in (1, 2, 40, 131, 5)]
        lens = [x.shape[0] for x in xs]
        norm = torch.from_numpy(PN.cmvn_norm(stats_of(np.concatenate(xs)), norm_vars=True)).cuda()
        feats = torch.from_numpy(np.concatenate(xs)).cuda()
        cfg = PostConfig(dim=D, delta_order=order, delta_window=window, left_context=L, right_context=R)
        K = D * (order + 1) * (L + R + 1)
        M = make_mat(rng, N, K, affine)
        Md = torch.from_numpy(M).cuda()
        fused = XformPlan(cfg, N, affine).compute(feats, lens, Md, norm=norm)
        rows = PostPlan(cfg).compute(feats, lens, norm=norm)              # cmvn | deltas | splice to HBM
        alone = XformPlan(PostConfig(dim=K), N, affine)                   # the stand-alone transform-feats
        assert (alone.in_dim, alone.tile >= 1) == (K, True)
        chained = alone.compute(rows, lens, Md)
        mm = torch.matmul(rows, Md[:, :K].T)
        if affine:
            mm = mm + Md[:, K]
        torch.cuda.synchronize()
        assert_bits_equal(fused.cpu().numpy(), chained.cpu().numpy(), (D, order, L, R, N))
        assert_within_bound(fused.cpu().numpy(), rows.cpu().numpy(), M, "fused")
        assert_within_bound(mm.cpu().numpy(), rows.cpu().numpy(), M, "torch.matmul")


CHECKS_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import test_transform as TT
from speech_recognition_tools_amd.plan import device_checks
from speech_recognition_tools_amd.post import PostConfig, XformPlan
assert device_checks(reset=True)[0], "not a checks build"
runs = 0
for D, order, window, L, R, N, affine in TT.CHECK_SHAPES:
    plan = XformPlan(PostConfig(dim=D, delta_order=order, delta_window=window, left_context=L, right_context=R),
                     N, affine)
    xs, norms, idx, mats, midx = TT.shape_case(D, order, window, L, R, N, affine, plan.tile, 1)
    got = TT.run_xform(plan, xs, mats, midx, norms, idx)
    assert np.all(np.isfinite(got))
    runs += 1
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": runs}))
"""
CHECK_SHAPES = [SHAPES[2], SHAPES[4], SHAPES[6]]


@pytest.mark.gpu
def test_gpu_device_range_checks_silent():
    """the FDLP_DEVICE_CHECKS build of xform_kernel: LDS, matrix and output indices of every tile stay in range"""
    import json
    import sys
    lib = os.path.join(ROOT, "speech_recognition_tools_amd", "lib", "libfdlp_checks.so")
    assert os.path.exists(lib), "build() compiles libfdlp_checks.so"
    r = subprocess.run([sys.executable, "-c", CHECKS_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=dict(os.environ, FDLP_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["enabled"] and res["runs"] == len(CHECK_SHAPES)
    assert res["violations"] == 0, res


def _write_ark(path, items, scp=None):
    from speech_recognition_tools_amd.post import FeatWriter
    w = FeatWriter("ark,scp:%s,%s" % (path, scp) if scp else "ark:" + path)
    for k, m in items:
        w.write(k, m)
    w.close()


@pytest.mark.gpu
def test_gpu_cli_pipe_fused_and_errors(tmp_path):
    from speech_recognition_tools_amd import cmvn, post
    from speech_recognition_tools_amd.cmvn import MatReader, write_table
    rng = np.random.default_rng(12)
    utts = [("s%d_u%d" % (i % 2, i), ark_like(rng, T, 13, float(i % 2))) for i, T in enumerate((5, 1, 90, 33, 1, 140))]
    d = str(tmp_path)
    feats, scp = d + "/feats.ark", d + "/feats.scp"
    _write_ark(feats, utts, scp)
    with open(d + "/utt2spk", "w") as f:
        f.writelines("%s %s\n" % (k, k.split("_")[0]) for k, _ in utts)
    with open(d + "/spk2utt", "w") as f:
        for s in ("s0", "s1"):
            f.write(s + " " + " ".join(k for k, _ in utts if k.startswith(s + "_")) + "\n")
    assert cmvn.main(["--spk2utt=ark:" + d + "/spk2utt", "scp:" + scp, "ark:" + d + "/cmvn.ark"]) == 0
    K = 13 * 9
    M = make_mat(rng, 40, K, False)
    write_fm(d + "/final.mat", M)
    copts = ["--norm-vars=true", "--utt2spk=ark:" + d + "/utt2spk"]
    sopts = ["--left-context=4", "--right-context=4"]
    # one process, one launch per batch
    assert post.main_post_feats(copts + ["--cmvn=ark:" + d + "/cmvn.ark"] + sopts + [
        "--transform=" + d + "/final.mat", "scp:" + scp, "ark,scp:%s/fused.ark,%s/fused.scp" % (d, d)]) == 0
    fused = open(d + "/fused.ark", "rb").read()
    # the stand-alone command on rows spliced before
    assert post.main_post_feats(copts + ["--cmvn=ark:" + d + "/cmvn.ark"] + sopts + [
        "scp:" + scp, "ark,scp:%s/c.ark,%s/c.scp" % (d, d)]) == 0
    assert post.main_transform_feats([d + "/final.mat", "scp:" + d + "/c.scp", "ark,scp:%s/t.ark,%s/t.scp" % (d, d)]) == 0
    assert open(d + "/t.ark", "rb").read() == fused
    # the rows are within the bound of the spliced rows
    spliced = dict((k, m.copy()) for k, m in MatReader("scp:" + d + "/c.scp"))
    got = dict((k, m.copy()) for k, m in MatReader("scp:" + d + "/fused.scp"))
    assert list(got) == [k for k, _ in utts]
    for k, _ in utts:
        assert_within_bound(got[k], spliced[k], M, k)
    # decode.sh's three-stage pipe through ark:-
    env = dict(os.environ)
    cmd = ("set -o pipefail; %s/apply-cmvn %s ark:%s/cmvn.ark scp:%s ark:- 2>%s/e1 | %s/splice-feats %s ark:- ark:- 2>%s/e2"
           " | %s/transform-feats %s/final.mat ark:- ark:%s/piped.ark 2>%s/e3"
           % (BIN, " ".join(copts), d, scp, d, BIN, " ".join(sopts), d, BIN, d, d, d))
    r = subprocess.run(["bash", "-c", cmd], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "".join(open(d + "/e%d" % i).read()[-1500:] for i in (1, 2, 3))
    assert open(d + "/piped.ark", "rb").read() == fused
    assert "Applied transform to 6 utterances; 0 had errors." in open(d + "/e3").read()

    # per-speaker fMLLR (affine, double matrices in a table): s1 has no matrix, s2's has K + 2 columns
    more = utts + [("s2_u0", ark_like(rng, 4, 13)), ("s2_u1", ark_like(rng, 9, 13))]
    _write_ark(d + "/more.ark", more, d + "/more.scp")
    with open(d + "/utt2spk2", "w") as f:
        f.writelines("%s %s\n" % (k, k.split("_")[0]) for k, _ in more)
    W = make_mat(rng, 13, 13, True).astype(np.float64)
    write_table("ark:" + d + "/trans.ark", [("s0", W), ("s2", rng.standard_normal((13, 15)))])
    r = subprocess.run([BIN + "/transform-feats", "--utt2spk=ark:" + d + "/utt2spk2", "ark:" + d + "/trans.ark",
                        "scp:" + d + "/more.scp", "ark,scp:%s/f.ark,%s/f.scp" % (d, d)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for k in ("s1_u1", "s1_u3", "s1_u5"):
        assert ("No fMLLR transform available for utterance %s, producing no output for this utterance" % k) in r.stderr
    for k in ("s2_u0", "s2_u1"):
        line = [l for l in r.stderr.splitlines() if k in l]
        assert len(line) == 1 and "13 x 15" in line[0] and "feat dim 13" in line[0], r.stderr[-2000:]
    assert "Applied transform to 3 utterances; 5 had errors." in r.stderr
    got = dict((k, m.copy()) for k, m in MatReader("scp:" + d + "/f.scp"))
    assert list(got) == ["s0_u0", "s0_u2", "s0_u4"]
    for k, x in utts[0::2]:
        assert_within_bound(got[k], x, W.astype(np.float32), k)
    # nothing written: exit status 1
    write_table("ark:" + d + "/bad.ark", [("s0", rng.standard_normal((13, 15)))])
    r = subprocess.run([BIN + "/transform-feats", "--utt2spk=ark:" + d + "/utt2spk2", "ark:" + d + "/bad.ark",
                        "scp:" + d + "/more.scp", "ark:" + d + "/none.ark"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stderr[-2000:]
    assert "Applied transform to 0 utterances; 8 had errors." in r.stderr
    assert not [f for f in os.listdir(d) if f.endswith(".tmp")]
