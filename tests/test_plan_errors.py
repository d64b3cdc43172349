"""Every plan create function refuses a bad configuration with the code and the message it always had, and
leaves no plan behind (csrc/fdlp_plan*.cpp).  Host-only: every row asks for device -1.

The rows are the rejections that fire after the plan object exists, where a create function has to give the
half-built plan back: while fdlp_plan_create's helper threads run (the filterbank kind), after them (lifter,
gamma weights, window), inside a nested create (a model plan whose chain is refused) and after one (the width
checks of the model plans).  Codes and messages are written out from the sources as they stood before the plan
layer was split by family.  fdlp_plan_create's "filterbank width nfft/2 does not match the frame length" has no
row: nfft = int(2 x) and N = int(x) for the same x = srate * fduration give floor(nfft / 2) = N for every x (and
int(x) / 2 = int(x / 2) in the complex mode), so no configuration reaches it.
"""
import ctypes

import numpy as np
import pytest

from speech_recognition_tools_amd import _lib
from speech_recognition_tools_amd.config import FeatureConfig

INVALID = _lib.FDLP_E_INVALID
FBANK_MSG = "Invalid type of filter bank, use mel or cochlear with proper configuration"
# dim 1000 spliced over -100000 .. +100000: 200001000 output columns, 4 bytes each
HUGE_POST = dict(dim=1000, left_context=100000, right_context=100000)
POST_MSG = ("post plan does not fit the 160 KB LDS at one frame per tile: dim 1000, delta order 0 window 0, "
            "context -100000..+100000 give 200001000 output columns and need %d bytes")


def _xform_msg(out_dim):
    # the staged matrix chunk: two chunks of 32 columns, min(ceil(out_dim / 16), 4) * 16 + 4 floats each
    extra = 4 * 2 * 32 * (min((out_dim + 15) // 16, 4) * 16 + 4)
    return (POST_MSG % (800004000 + extra)) + " (with a transform to %d columns, %d of the bytes)" % (out_dim, extra)


def _post(dim=40, **over):
    c = _lib.FdlpPostConfigC()
    c.dim, c.device = dim, -1
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _fdlp(**over):
    lifter = over.pop("lifter", None)
    c, keep = FeatureConfig(lifter=lifter).to_c(max_frames=4)
    for k, v in over.items():
        setattr(c, k, v)
    return lambda out: (_lib.lib.fdlp_plan_create(ctypes.byref(c), -1, out), keep)[0]


def _mel(**over):
    c = _lib.FdlpMelConfigC()
    c.nfilters, c.nfft, c.frate, c.srate, c.fduration, c.warp_fact, c.max_frames = 20, 512, 100, 16000, 0.025, 1.0, 4
    for k, v in over.items():
        setattr(c, k, v)
    return lambda out: _lib.lib.fdlp_mel_plan_create(ctypes.byref(c), -1, out)


def _mfcc(**over):
    c = _lib.FdlpMfccConfigC()
    c.nfilters, c.nfft, c.frate, c.srate, c.fduration, c.max_frames = 20, 512, 100, 16000, 0.025, 4
    for k, v in over.items():
        setattr(c, k, v)
    return lambda out: _lib.lib.fdlp_mfcc_plan_create(ctypes.byref(c), -1, out)


def _post_plan(**over):
    c = _post(**over)
    return lambda out: _lib.lib.fdlp_post_plan_create(ctypes.byref(c), out)


def _xform(out_dim, **over):
    c = _lib.FdlpXformConfigC()
    c.post, c.out_dim, c.affine = _post(**over), out_dim, 1
    return lambda out: _lib.lib.fdlp_xform_plan_create(ctypes.byref(c), out)


def _rnn(dims, **over):
    c = _lib.FdlpRnnConfigC()
    c.post, c.n_stages = _post(**over), len(dims) - 1
    for s in range(c.n_stages):
        c.kind[s] = _lib.FDLP_RNN_LINEAR
    for s, d in enumerate(dims):
        c.dims[s] = d
    return lambda out: _lib.lib.fdlp_rnn_plan_create(ctypes.byref(c), None, 16, 1, out)


def _nnet(dims, **over):
    c = _lib.FdlpNnetConfigC()
    c.post, c.n_linear = _post(**over), len(dims) - 1
    for s, d in enumerate(dims):
        c.dims[s] = d
    return lambda out: _lib.lib.fdlp_nnet_plan_create(ctypes.byref(c), None, None, 16, out)


def _mmod(stream1):
    c = _lib.FdlpMmodConfigC()
    c.n_streams, c.in_dim, c.n_sub_layers, c.hidden_sub, c.n_trunk_layers, c.n_classes = 2, 40, 1, 8, 0, 5
    c.post[0], c.post[1] = _post(), _post(**stream1)
    return lambda out: _lib.lib.fdlp_mmod_plan_create(ctypes.byref(c), None, 16, 1, out)


CASES = [
    ("fdlp_plan_create-mode", _fdlp(mode=5), INVALID, "unknown plan mode"),
    ("fdlp_plan_create-fbank-kind", _fdlp(fbank_kind=7), INVALID, FBANK_MSG),
    ("fdlp_plan_create-lifter-length", _fdlp(lifter=np.ones(49)), INVALID,
     "lifter_config must hold coeff_num values (reference broadcast)"),
    ("fdlp_plan_create-gamma-order", _fdlp(gamma_enabled=1, gamma_scale=1.0, gamma_shape=2.0, order=40), INVALID,
     "gamma_weight has length order and needs order == coeff_num (reference broadcast)"),
    ("fdlp_plan_create-window", _fdlp(window=9), INVALID, "unknown analysis window"),
    ("fdlp_mel_plan_create-nfft", _mel(nfft=22), INVALID, "nfft/2 must factor into 2, 3, 5 and 7"),
    ("fdlp_mel_plan_create-fbank-kind", _mel(fbank_kind=7), INVALID, FBANK_MSG),
    ("fdlp_mfcc_plan_create-tile", _mfcc(nfft=8192, fduration=0.5), INVALID,
     "mfcc tile exceeds the 160 KB LDS: need max(min(L, n), nfilters) + n/2 <= ~1230 "
     "(n = nfft/2 + 1, L = srate * fduration)"),
    ("fdlp_post_plan_create-lds", _post_plan(**HUGE_POST), INVALID, POST_MSG % 800004000),
    ("fdlp_xform_plan_create-lds", _xform(40, **HUGE_POST), INVALID, _xform_msg(40)),
    ("fdlp_rnn_plan_create-width", _rnn([39, 10]), INVALID,
     "the model's input dimension dims[0] = 39 differs from the 40 columns the stages before it give"),
    ("fdlp_rnn_plan_create-chain", _rnn([1000, 10], **HUGE_POST), INVALID, _xform_msg(10)),
    ("fdlp_nnet_plan_create-width", _nnet([39, 10]), INVALID,
     "the network's input dimension dims[0] = 39 differs from the 40 columns the stages before it give"),
    ("fdlp_mmod_plan_create-width", _mmod(dict(dim=80)), INVALID,
     "stream 1 gives 80 spliced columns where the sub-networks take in_dim = 40"),
    ("fdlp_mmod_plan_create-chain", _mmod(HUGE_POST), INVALID, "stream 1: " + _xform_msg(24)),
]


@pytest.mark.parametrize("create,code,message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_create_refuses(create, code, message):
    out = ctypes.c_void_p(0xdead)  # create clears it before anything else
    assert create(ctypes.byref(out)) == code
    assert _lib.lib.fdlp_last_error().decode() == message
    assert not out.value


def test_every_create_function_has_a_row():
    creates = {n for n in _lib.SIGNATURES if n.endswith("_plan_create")}
    assert creates == {c[0].split("-")[0] for c in CASES}
