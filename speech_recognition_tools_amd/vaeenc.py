"""The VAE-encoded GRU models of the hybrid recipes on the MI355X: a drop-in for the reference's
src/nnet/compute_vae_encoded_likelihood.py (recipes/timit/local_pyspeech/decode_dnn_vae_encoded.sh), which pushes
the `apply-cmvn --norm-vars=true | splice-feats` rows of one utterance at a time through a VAE encoder and a GRU
classifier in torch on the CPU.  Per utterance:

  1. the VAE encoder.  --vae_arch=cnn (the default) is VAECNNEncoderNopool (nnet_models_cnn.py:180-207): same-padded
     Conv2d + ReLU layers over the (feature x time) image, flattened to C_last F per frame; anything else is
     VAEEncoder (nnet_models.py:262-297), a GRU stack;
  2. `means`, a Conv1d of kernel size 1, gives the latent z [T, bn].  Only the means are kept: the script throws
     the sampled decoder output away, so it is deterministic, and `vars` and every decoder key are ignored here;
  3. z - mean_t(z), divided by sqrt(var_t(.)), unbiased, per utterance (:128-129);
  4. nnetRNN(bn, num_layers, hidden_dim, num_classes) on it;
  5. logits, softmax, or log_softmax - prior_weight * prior.

A convolution is one launch of conv2d_same_kernel, the normaliser of utt_norm_kernel (csrc/fdlp_vaeenc.hip,
include/fdlp.h); everything else is the stage plan of rnn.py, whose StagePlan, runner and command-line body this
module uses.  Every value is computed in an order fixed by the model's shape and the utterance's length alone, so
the files do not depend on --batch-rows.

Divergences from the reference, on purpose:
  * A ONE-FRAME utterance is warned about by name, counted as an error and NOT written.  Its unbiased variance is
    0 / 0, so the reference writes rows of NaN, which the decoder cannot use.  (The plan itself has no special
    case: it gives the NaN.)
  * vae_type "arvae" with --vae_arch=cnn crashes in the reference (it builds the GRU nnetARVAE and feeds it a 4-D
    image); here it exits 1 with a message.
  * The encoder file is nnet['vaeenc'], relative to the working directory as in the reference, or --vaeenc.
  * The reference's `print(batch_x.shape)` to stdout is not reproduced; --max_seq_len is accepted and unused, as there.
  * --add_softmax uses the max-subtracted form nnet.py documents.
  * The GRU scan holds at most 384 hidden units (the trainer's default hidden_dim is 512): the plan's message says so.

--batch-rows defaults to 32768: the two stage workspaces are [rows, max_l C_l F] float32, 1664 columns for the
trainer's default 1 -> 32 -> 64 -> 128 at F = 13, so 32768 rows are 0.44 GB of workspace (beside 0.1 GB of GRU
projections), and still hold more than one full scan group (32 utterances) of 8-second utterances.
"""
import argparse
import ctypes
import dataclasses
import os
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import FdlpVencConfigC, check, lib, ptr
from .nnet import StagePlan, _load_prior, open_checkpoint, run_model_tool, state_array
from .post import MatReader, PostConfig
from .rnn import RnnRunner, _gru_stages, load_rnn_egs_config


@dataclass
class VaeEncShape:
    """what the library needs of a model: arch "rnn" (in_dim, n_enc_layers, enc_hidden) or "cnn" (channels [1, ..],
    kh, kw, feat_h), then latent_dim, n_cls_layers, cls_hidden, n_classes"""
    arch: str
    latent_dim: int
    n_cls_layers: int
    cls_hidden: int
    n_classes: int
    in_dim: int = 0
    n_enc_layers: int = 0
    enc_hidden: int = 0
    channels: Sequence[int] = ()
    kh: int = 0
    kw: int = 0
    feat_h: int = 0

    @property
    def kinds(self):
        enc = ["conv"] * (len(self.channels) - 1) if self.arch == "cnn" else ["gru"] * self.n_enc_layers
        return enc + ["linear", "norm"] + ["gru"] * self.n_cls_layers + ["linear"]


def shape_of_stages(stages) -> VaeEncShape:
    """the shape of a stage list: ("conv", w [Co, Ci, kh, kw], b) or ("gru", w_ih, w_hh, b_ih, b_hh) encoder stages,
    ("linear", w, b) the means, ("norm",), classifier GRUs, ("linear", w, b) the regression"""
    kinds = [st[0] for st in stages]
    if "norm" not in kinds or kinds.count("norm") != 1:
        raise ValueError("VaeEncPlan: the stages need exactly one ('norm',)")
    n = kinds.index("norm")
    enc, cls = stages[:n - 1], stages[n + 1:-1]
    arch = "cnn" if kinds[0] == "conv" else "rnn"
    if (n < 2 or kinds[n - 1] != "linear" or kinds[-1] != "linear" or not cls
            or any(k != ("conv" if arch == "cnn" else "gru") for k in kinds[:n - 1])
            or any(k != "gru" for k in kinds[n + 1:-1])):
        raise ValueError("VaeEncPlan: the stages must be encoder (conv.. or gru..), linear, norm, gru.., linear; got %s"
                         % kinds)
    sh = VaeEncShape(arch, int(np.shape(stages[n - 1][1])[0]), len(cls), int(np.shape(cls[0][2])[1]),
                     int(np.shape(stages[-1][1])[0]))
    if arch == "cnn":
        w0 = np.shape(enc[0][1])
        if any(len(np.shape(st[1])) != 4 for st in enc):
            raise ValueError("VaeEncPlan: a conv stage's weight is [Co, Ci, kh, kw]")
        sh.channels = [int(w0[1])] + [int(np.shape(st[1])[0]) for st in enc]
        sh.kh, sh.kw = int(w0[2]), int(w0[3])
        k_means = int(np.shape(stages[n - 1][1])[1])
        if sh.channels[-1] < 1 or k_means % sh.channels[-1]:
            raise ValueError("VaeEncPlan: the means take %d columns, which are not whole rows of %d channels"
                             % (k_means, sh.channels[-1]))
        sh.feat_h = k_means // sh.channels[-1]
    else:
        sh.in_dim, sh.n_enc_layers, sh.enc_hidden = int(np.shape(enc[0][1])[1]), len(enc), int(np.shape(enc[0][2])[1])
    return sh


class VaeEncPlan(StagePlan):
    """cmvn | deltas | splice | VAE encoder | means | per-utterance normaliser | GRU classifier | regression.
    stages: see shape_of_stages; the ReLU after a conv stage is applied when the next stage loads its output, so
    tapping it gives the pre-activation.  device=-1 gives a host-only plan (dims, workspace_bytes, group_utts,
    lds_bytes = (gru_scan_kernel, conv2d_same_kernel), groups()); it needs the shape only: stages=None with `shape`."""
    _DESTROY, _COMPUTE = "fdlp_venc_plan_destroy", "fdlp_venc_compute"

    def __init__(self, cfg: PostConfig, stages, max_rows: int = 32768, max_utts: Optional[int] = None,
                 device: int = 0, shape: Optional[VaeEncShape] = None):
        self.cfg, self.device, self.max_rows = cfg, int(device), int(max_rows)
        self.max_utts = int(max_utts) if max_utts is not None else max(1, self.max_rows)
        arrays = None
        if stages is not None:
            shape = shape_of_stages(stages)
            arrays, want_k = [], None
            for s, st in enumerate(stages):
                a = [np.ascontiguousarray(x, dtype=np.float32) for x in st[1:]]
                if st[0] == "gru" and len(a) == 4:
                    H = a[1].shape[1] if a[1].ndim == 2 else -1
                    if (a[0].ndim != 2 or a[0].shape[0] != 3 * H or a[1].shape != (3 * H, H) or a[2].shape != (3 * H,)
                            or a[3].shape != (3 * H,)):
                        raise ValueError("VaeEncPlan: GRU stage %d has shapes %s" % (s, [x.shape for x in a]))
                    k_in, n_out, four = a[0].shape[1], H, a
                elif st[0] == "linear" and len(a) == 2:
                    if a[0].ndim != 2 or a[1].shape != (a[0].shape[0],):
                        raise ValueError("VaeEncPlan: linear stage %d has weight %s and bias %s"
                                         % (s, a[0].shape, a[1].shape))
                    k_in, n_out, four = a[0].shape[1], a[0].shape[0], [a[0], None, a[1], None]
                elif st[0] == "conv" and len(a) == 2:
                    if a[0].ndim != 4 or a[0].shape[2:] != (shape.kh, shape.kw) or a[1].shape != (a[0].shape[0],):
                        raise ValueError("VaeEncPlan: conv stage %d has weight %s and bias %s for a kernel (%d, %d)"
                                         % (s, a[0].shape, a[1].shape, shape.kh, shape.kw))
                    k_in, n_out = a[0].shape[1] * shape.feat_h, a[0].shape[0] * shape.feat_h
                    four = [a[0], None, a[1], None]
                elif st[0] == "norm" and not a:
                    k_in = n_out = want_k
                    four = [None] * 4
                else:
                    raise ValueError("VaeEncPlan: stage %d is %r with %d arrays" % (s, st[0], len(a)))
                if want_k is not None and k_in != want_k:
                    raise ValueError("VaeEncPlan: stage %d takes %d columns after a stage of %d outputs"
                                     % (s, k_in, want_k))
                want_k = n_out
                arrays += four
        if shape is None:
            raise ValueError("VaeEncPlan: stages or shape")
        self.shape = shape
        c = FdlpVencConfigC()
        c.post = cfg.to_c(device)
        c.arch = _lib.FDLP_VENC_CNN if shape.arch == "cnn" else _lib.FDLP_VENC_RNN
        c.in_dim, c.n_enc_layers, c.enc_hidden = int(shape.in_dim), int(shape.n_enc_layers), int(shape.enc_hidden)
        c.n_conv = max(len(shape.channels) - 1, 0)
        for i, ch in enumerate(list(shape.channels)[:_lib.FDLP_VENC_MAX_CONV + 1]):
            c.channels[i] = int(ch)
        c.kh, c.kw, c.feat_h = int(shape.kh), int(shape.kw), int(shape.feat_h)
        c.latent_dim, c.n_cls_layers = int(shape.latent_dim), int(shape.n_cls_layers)
        c.cls_hidden, c.n_classes = int(shape.cls_hidden), int(shape.n_classes)
        pp = None
        if arrays is not None:
            pp = (ctypes.c_void_p * len(arrays))(*[a.ctypes.data if a is not None else None for a in arrays])
        h = ctypes.c_void_p()
        check(lib.fdlp_venc_create(ctypes.byref(c), pp, self.max_rows, self.max_utts, ctypes.byref(h)))
        self._h = h
        ind, ns, gu = _lib.c_i32(), _lib.c_i32(), _lib.c_i32()
        wsb = _lib.c_i64()
        lds = (_lib.c_i32 * 2)()
        od = (_lib.c_i32 * _lib.FDLP_RNN_MAX_STAGES)()
        check(lib.fdlp_venc_plan_info(self._h, ctypes.byref(ind), ctypes.byref(ns), od, ctypes.byref(wsb),
                                      ctypes.byref(gu), lds))
        self.in_dim, self.n_stages = ind.value, ns.value
        self.dims = [ind.value] + [od[i] for i in range(ns.value)]
        self.kinds = shape.kinds
        self.out_dim = self.dims[-1]
        self.workspace_bytes, self.group_utts, self.lds_bytes = wsb.value, gu.value, (lds[0], lds[1])

    def groups(self, lengths: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, int]:
        """(group_of, slot_of, n_groups) of a batch with these lengths, as RnnPlan.groups"""
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32))
        g, s = np.zeros(lens.size, dtype=np.int32), np.zeros(lens.size, dtype=np.int32)
        n = _lib.c_i32()
        check(lib.fdlp_venc_plan_groups(self._h, ptr(lens, ctypes.c_int32), lens.size, ptr(g, ctypes.c_int32),
                                        ptr(s, ctypes.c_int32), ctypes.byref(n)))
        return g, s, n.value

    def set_profiling(self, on: bool):
        check(lib.fdlp_venc_set_profiling(self._h, int(bool(on))))

    def times(self):
        """(ms in the projections, linear stages and the normaliser, ms in the scans, ms in the convolutions) since
        the last call; waits for them"""
        ms = (ctypes.c_double * 3)()
        check(lib.fdlp_venc_times(self._h, ms))
        return ms[0], ms[1], ms[2]


# ---------------------------------------------------------------------------------------------
# the reference's checkpoints: the classifier dict of train_VAE_encoded_nnet_classfier.py and the encoder file it names
# ---------------------------------------------------------------------------------------------
@dataclass
class VaeEncCheckpoint:
    vae_arch: str        # "cnn" or "rnn"
    vae_type: str
    feature_dim: int     # what the runner checks the features against: the encoder's feature_dim (cnn: the image height)
    num_frames: int      # spliced frames (cnn: 1; the header's num_frames there is the training chunk's width)
    num_classes: int
    header: dict
    enc_header: dict
    vaeenc: str          # the encoder file that was read
    stages: List[tuple] = field(default_factory=list)

    num_layers = 0   # NnetRunner's --layer check: only the last stage is written

    @property
    def dims(self):
        out, k = [], None
        for s in self.stages:
            k = (s[2].shape[1] if s[0] == "gru" else k if s[0] == "norm"
                 else s[1].shape[0] * self.feature_dim * self.num_frames if s[0] == "conv" else s[1].shape[0])
            out.append(k)
        return [self.feature_dim * self.num_frames] + out


CLS_KEYS = ("num_layers", "hidden_dim", "num_classes")
ENC_RNN_KEYS = ("feature_dim", "num_frames", "encoder_num_layers", "hidden_dim")
ENC_CNN_KEYS = ("feature_dim", "num_frames")


def _comma_ints(path, d, key, n=None):
    if key not in d:
        raise ValueError("%s: the checkpoint has no key '%s' (--vae_arch=cnn)" % (path, key))
    try:
        v = [int(x) for x in str(d[key]).split(",")]
    except ValueError:
        raise ValueError("%s: key '%s' is not a comma-separated list of integers (%r)" % (path, key, d[key]))
    if (n is not None and len(v) != n) or any(x < 1 for x in v):
        raise ValueError("%s: key '%s' is %r" % (path, key, d[key]))
    return v


def _sub_state(sd, prefix):
    """the keys of sd under `prefix`, without it: a view the shared readers take"""
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def load_vaeenc_checkpoint(model_path: str, vae_arch: str = "cnn", vaeenc: Optional[str] = None) -> VaeEncCheckpoint:
    """torch.load of the classifier dict (vaeenc, vae_type, num_layers, hidden_dim, num_classes; model_state_dict is
    nnetRNN's: layers.{i}.*_l0, regression.*) and of the encoder file it names (`vaeenc` overrides the header's
    path).  Encoder headers: RNN feature_dim, num_frames, encoder_num_layers, hidden_dim, bn_dim; CNN feature_dim,
    num_frames, in_channels, out_channels, kernel as comma strings, bn_dim; with vae_type "modulation" the latent
    width is nfilters * nrepeats.  Of its model_state_dict only vae_encoder.layers.{i}.* or vae_encoder.cnn_layers.{i}.*
    and vae_encoder.means.* are read; vae_encoder.vars.* and every vae_decoder.* key are ignored.  Every shape is
    checked against the headers; the errors name the file and the key."""
    arch = "cnn" if vae_arch == "cnn" else "rnn"
    hdr, sd, top = open_checkpoint(model_path, CLS_KEYS, whole=True)
    for k in ("vaeenc", "vae_type"):
        if k not in top:
            raise ValueError("%s: the checkpoint has no key '%s'" % (model_path, k))
    vae_type = str(top["vae_type"])
    if vae_type == "arvae" and arch == "cnn":
        raise ValueError("%s: vae_type 'arvae' has a GRU encoder; --vae_arch=cnn cannot run it (the reference "
                         "crashes there)" % model_path)
    enc_path = vaeenc if vaeenc is not None else str(top["vaeenc"])
    ehdr, esd, etop = open_checkpoint(enc_path, ENC_CNN_KEYS if arch == "cnn" else ENC_RNN_KEYS,
                                      hint=" (--vae_arch=%s)" % vae_arch, whole=True)
    lat_keys = ("nfilters", "nrepeats") if vae_type == "modulation" else ("bn_dim",)
    for k in lat_keys:
        if k not in etop:
            raise ValueError("%s: the checkpoint has no key '%s' (vae_type %s)" % (enc_path, k, vae_type))
        try:
            ehdr[k] = int(etop[k])
        except (TypeError, ValueError):
            raise ValueError("%s: key '%s' is not an integer (%r)" % (enc_path, k, etop[k]))
        if ehdr[k] < 1:
            raise ValueError("%s: key '%s' is %d" % (enc_path, k, ehdr[k]))
    bn = ehdr["nfilters"] * ehdr["nrepeats"] if vae_type == "modulation" else ehdr["bn_dim"]
    enc = _sub_state(esd, "vae_encoder.")
    F = ehdr["feature_dim"]
    stages = []
    if arch == "cnn":
        kh, kw = _comma_ints(enc_path, etop, "kernel", 2)
        cin = _comma_ints(enc_path, etop, "in_channels")
        cout = _comma_ints(enc_path, etop, "out_channels")
        ehdr.update(kernel="%d,%d" % (kh, kw), in_channels=",".join(map(str, cin)), out_channels=",".join(map(str, cout)))
        if len(cin) != len(cout) or any(a != b for a, b in zip(cin[1:], cout[:-1])):
            raise ValueError("%s: 'in_channels' %s and 'out_channels' %s do not chain"
                             % (enc_path, etop["in_channels"], etop["out_channels"]))
        shown = {k: v for k, v in ehdr.items() if isinstance(v, int)}
        for i, (ci, co) in enumerate(zip(cin, cout)):
            name = "cnn_layers.%d." % i
            w = _enc_array(enc_path, enc, name + "weight", (co, ci, kh, kw), shown)
            stages.append(("conv", w, _enc_array(enc_path, enc, name + "bias", (co,), shown)))
        extra = [k for k in enc if k.startswith("cnn_layers.") and k.split(".")[1].isdigit()
                 and int(k.split(".")[1]) >= len(cin)]
        if extra:
            raise ValueError("%s: model_state_dict has 'vae_encoder.%s' beyond the %d layers of the header"
                             % (enc_path, extra[0], len(cin)))
        k_means, feature_dim, num_frames = cout[-1] * F, F, 1
    else:
        H = ehdr["hidden_dim"]
        try:
            stages += _gru_stages(enc_path, enc, "layers", ehdr["encoder_num_layers"], F * ehdr["num_frames"], H, ehdr)
        except ValueError as e:   # the shared reader names the key without the prefix it never saw
            raise ValueError(str(e).replace("'layers.", "'vae_encoder.layers."))
        k_means, feature_dim, num_frames = H, F, ehdr["num_frames"]
    shown = {k: v for k, v in ehdr.items() if isinstance(v, int)}
    stages.append(("linear", _enc_array(enc_path, enc, "means.weight", (bn, k_means), shown, conv1d=True),
                   _enc_array(enc_path, enc, "means.bias", (bn,), shown)))
    stages.append(("norm",))
    Hc, C = hdr["hidden_dim"], hdr["num_classes"]
    stages += _gru_stages(model_path, sd, "layers", hdr["num_layers"], bn, Hc, hdr)
    stages.append(("linear", state_array(model_path, sd, "regression.weight", (C, Hc), hdr, conv1d=True),
                   state_array(model_path, sd, "regression.bias", (C,), hdr)))
    return VaeEncCheckpoint(arch, vae_type, feature_dim, num_frames, C, hdr, ehdr, enc_path, stages)


def _enc_array(path, enc, name, want, shown, conv1d=False):
    try:
        return state_array(path, enc, name, want, shown, conv1d=conv1d)
    except ValueError as e:
        raise ValueError(str(e).replace("'%s'" % name, "'vae_encoder.%s'" % name))


# ---------------------------------------------------------------------------------------------
# runner: RnnRunner around a VaeEncPlan; one-frame utterances are skipped
# ---------------------------------------------------------------------------------------------
class VaeEncRunner(RnnRunner):
    BATCH_ROWS, PROG = 32768, "compute-vae-encoded-likelihood"

    def __init__(self, ckpt, egs, **kw):
        if ckpt.vae_arch == "cnn":
            # the image height is the width of the spliced rows: the raw features are feature_dim / frames wide
            frames = egs.left + egs.right + 1
            if ckpt.feature_dim % frames:
                raise ValueError("the CNN encoder takes images of height %d, which egs.config's splice -%d..+%d of %d "
                                 "frames cannot give" % (ckpt.feature_dim, egs.left, egs.right, frames))
            ckpt = dataclasses.replace(ckpt, feature_dim=ckpt.feature_dim // frames, num_frames=frames)
        super().__init__(ckpt, egs, **kw)

    def _new_plan(self, cfg, rows):
        return VaeEncPlan(cfg, self.ckpt.stages, max_rows=rows, max_utts=rows, device=self.device)

    def _reader(self, rspecifier):
        for utt, m in MatReader(rspecifier):
            if m.shape[0] == 1:
                self.log("Utterance %s has one frame: the variance of its latent over time is undefined, producing no "
                         "output for this utterance" % utt)
                self.num_err += 1
                continue
            yield utt, m


# ---------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------
def compute_vae_encoded_likelihood_parser():
    ap = argparse.ArgumentParser(prog="compute-vae-encoded-likelihood",
                                 description="Logits, posteriors or pseudo log-likelihoods of a GRU classifier on a VAE encoder's "
                                 "normalised latent, on the MI355X")
    ap.add_argument("model", help="checkpoint of the classifier; its header names the VAE encoder file")
    ap.add_argument("scp", help="feats.scp of the JOB (or an ark: / scp: rspecifier)")
    ap.add_argument("egs_config", help="the egs.config pickle written at data preparation")
    ap.add_argument("save_file", help="output base name: <save_file>.ark and .scp are written (or an ark wspecifier)")
    ap.add_argument("--vae_arch", default="cnn", help="encoder family: cnn (Conv2d stack); anything else is the GRU stack")
    ap.add_argument("--max_seq_len", default=512, type=int, help="accepted and unused, as in the reference")
    ap.add_argument("--prior", default=None, help="pickle of the log prior [num_classes]: write log_softmax - prior_weight * prior")
    ap.add_argument("--prior_weight", type=float, default=0.8, help="weight of the prior (default 0.8)")
    ap.add_argument("--add_softmax", action="store_true", help="write softmax posteriors instead of logits (ignored with --prior)")
    ap.add_argument("--override_trans", default=None, help="<pca|cmvn|cmvn_utt>,<path> to use instead of egs.config's feat_type")
    ap.add_argument("--vaeenc", default=None, help="the VAE encoder file, instead of the path in the model's header")
    ap.add_argument("--ark_precision", type=int, default=3, help="decimals of the written values, like the "
                    "reference's '%%.3f' text ark; negative keeps float32")
    ap.add_argument("--device", type=int, default=int(os.environ.get("FDLP_DEVICE", "0")))
    ap.add_argument("--batch-rows", type=int, default=VaeEncRunner.BATCH_ROWS,
                    help="rows per device batch (whole utterances)")
    return ap


def main_compute_vae_encoded_likelihood(argv=None):
    prog = "compute-vae-encoded-likelihood"
    a = compute_vae_encoded_likelihood_parser().parse_args(argv)

    def make_runner():
        ckpt = load_vaeenc_checkpoint(a.model, a.vae_arch, a.vaeenc)
        egs = load_rnn_egs_config(a.egs_config, a.override_trans)
        mode, prior = "raw", None
        if a.prior:
            mode, prior = "loglike", _load_prior(a.prior)
        elif a.add_softmax:
            mode = "softmax"
        return VaeEncRunner(ckpt, egs, mode=mode, prior=prior, prior_weight=a.prior_weight, device=a.device,
                            batch_rows=a.batch_rows, decimals=a.ark_precision, prog=prog)

    return run_model_tool(prog, a, make_runner, "Computed likelihoods")


if __name__ == "__main__":
    sys.exit(main_compute_vae_encoded_likelihood(sys.argv[1:]))
