"""The multi-stream GRU acoustic model of the TIMIT recipe on the MI355X: a drop-in for the reference's
src/nnet/dump_multimod_outputs.py (recipes/timit/local_pyspeech/decode_multimod_dnn.sh), which pushes one utterance
at a time through nnetRNNMultimod (nnet_models.py:92-161) on the CPU.  The model has one GRU sub-network per
modulation-spectrum stream (the recipe's modspec_20_1_15_0.5_{15,25,35}, what compute-modspec-feats writes); the
sub-network outputs, side by side, pass through trunk GRUs and a regression layer (a Conv1d of kernel size 1).

  * Every GRU layer is rnn.py's: the input projection of all rows at once (layer 0's inside its stream's chain
    launch), then gru_scan_kernel.  The scans of the M sub-networks are independent recurrences of one width over
    the same utterances, so each sub-network layer is ONE launch on the grid (groups, streams) that keeps M times
    as many CUs busy as a single-stream scan, and the last one writes stream s at column s Hs of the [rows, M Hs]
    buffer the trunk reads: torch.cat never happens as a copy (include/fdlp.h).  An utterance's bits do
    not depend on the batch, so the files do not depend on --batch-rows.
  * The trunk GRUs are M Hs wide and the scan holds its state twice in LDS: M Hs <= 384 (the recipe's 3 x 100 fits;
    3 x 256 is refused at plan creation with both numbers in the message).

Decisions where the reference is broken or silent:
  * The reference hard-codes three streams (`batch_x1, batch_x2, batch_x3`).  This tool takes any mod_num in 1 .. 8;
    the counts of `scps` and `egs_configs` must equal mod_num, else exit 1 with the reference's messages.
  * A feat type that is none of pca / cmvn / cmvn_utt crashes the reference (it formats `config.scp`, which does
    not exist).  Here it means raw features of that stream.  pca, cmvn (--norm-vars=true) and cmvn_utt are handled
    per stream exactly as dump-genclassifier-outputs handles them (rnn.RnnRunner).
  * --override_trans is parsed and never used by the reference: accepted, ignored, and warned about once.
  * `concat_feats` is required in every egs.config (the reference splits it unconditionally).
  * Utterances are taken in stream 0's order.  The reference crashes (KeyError) on an utterance missing from
    another stream and (torch.cat) on one whose frame counts differ between streams; here each is warned about,
    counted as an error and skipped.  The other streams are read in step with stream 0; an utterance that is not
    the next one of its table is looked for further on, and what was passed over is kept for later.
  * --add_softmax uses the max-subtracted form nnet.py documents; failures leave no partial files behind.
Out of scope: training.

The checkpoint and egs.config readers, the two-slot loop and the command line's body are nnet.py's and rnn.py's
(open_checkpoint, _gru_stages, load_rnn_egs_config, RnnRunner, run_model_tool); this module adds the multi-stream
plan, the checkpoint's layout and the lock-step reading of M tables.
"""
import argparse
import ctypes
import os
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import FdlpMmodConfigC, FdlpPostBatchC, check, lib, ptr
from .cmvn import MatReader
from .nnet import MODES, _load_prior, open_checkpoint, run_model_tool
from .post import PostConfig, _make_batch
from .rnn import RnnRunner, _gru_stages, _state_array, load_rnn_egs_config

MAX_STREAMS = _lib.FDLP_MMOD_MAX_STREAMS


def _gru_arrays(who, what, layer, k_in):
    """the four float32 arrays of one nn.GRU layer, checked: (w_ih [3H, k_in], w_hh [3H, H], b_ih [3H], b_hh [3H])"""
    if len(layer) != 4:
        raise ValueError("%s: %s must be (w_ih, w_hh, b_ih, b_hh)" % (who, what))
    w_ih, w_hh, b_ih, b_hh = (np.ascontiguousarray(x, dtype=np.float32) for x in layer)
    H = w_hh.shape[1] if w_hh.ndim == 2 else -1
    if (w_ih.shape != (3 * H, k_in) or w_hh.shape != (3 * H, H) or b_ih.shape != (3 * H,) or b_hh.shape != (3 * H,)):
        raise ValueError("%s: %s has shapes %s, %s, %s, %s for %d input columns"
                         % (who, what, w_ih.shape, w_hh.shape, b_ih.shape, b_hh.shape, k_in))
    return [w_ih, w_hh, b_ih, b_hh], H


class MultimodPlan:
    """M chains (cmvn | deltas | splice, cfgs[s]) | M GRU sub-networks | trunk GRUs | regression.
    subnets[s][i], trunk[l]: (w_ih, w_hh, b_ih, b_hh) in nn.GRU's layout; regression: (w [C, M Hs], b [C]).  Every
    stream's chain must give the sub-networks' input width.  device=-1 gives a host-only plan (in_dim, tap dims,
    workspace_bytes, group_utts, lds_bytes, groups()); it needs the shapes only: pass subnets=None with
    shape=(in_dim, n_sub_layers, hidden_sub, n_trunk_layers, n_classes).
    Taps: 0 the logits; 1 .. n_trunk_layers the trunk GRUs counted from the end; n_trunk_layers + 1 the
    concatenated sub-network outputs [rows, M Hs]."""

    def __init__(self, cfgs: Sequence[PostConfig], subnets, trunk=(), regression=None, max_rows: int = 131072,
                 max_utts: Optional[int] = None, device: int = 0, shape: Optional[Sequence[int]] = None):
        who = "MultimodPlan"
        self.cfgs, self.device, self.max_rows = list(cfgs), int(device), int(max_rows)
        self.max_utts = int(max_utts) if max_utts is not None else max(1, self.max_rows)
        M = self.n_streams = len(self.cfgs)
        arrays = None
        if subnets is not None:
            if len(subnets) != M or not M or regression is None:
                raise ValueError("%s: one sub-network per stream (%d for %d streams) and a regression layer"
                                 % (who, len(subnets), M))
            Ls = len(subnets[0])
            if not Ls or any(len(sn) != Ls for sn in subnets):
                raise ValueError("%s: every sub-network needs the same number (>= 1) of layers" % who)
            arrays, Hs = [], None
            in_dim = np.asarray(subnets[0][0][0]).shape[-1]
            for s, sn in enumerate(subnets):
                for i, layer in enumerate(sn):
                    a, H = _gru_arrays(who, "layer %d of sub-network %d" % (i, s), layer, in_dim if i == 0 else Hs or -1)
                    Hs = H if Hs is None else Hs
                    if H != Hs:
                        raise ValueError("%s: layer %d of sub-network %d has %d hidden units, the others %d"
                                         % (who, i, s, H, Hs))
                    arrays += a
            for l, layer in enumerate(trunk):
                a, H = _gru_arrays(who, "trunk layer %d" % l, layer, M * Hs)
                if H != M * Hs:
                    raise ValueError("%s: trunk layer %d has %d hidden units for %d streams of %d" % (who, l, H, M, Hs))
                arrays += a
            w, b = (np.ascontiguousarray(x, dtype=np.float32) for x in regression)
            if w.ndim != 2 or w.shape[1] != M * Hs or b.shape != (w.shape[0],):
                raise ValueError("%s: the regression has weight %s and bias %s for %d streams of %d"
                                 % (who, w.shape, b.shape, M, Hs))
            arrays += [w, b]
            shape = (in_dim, Ls, Hs, len(trunk), w.shape[0])
        if shape is None or len(shape) != 5:
            raise ValueError("%s: shape must be (in_dim, n_sub_layers, hidden_sub, n_trunk_layers, n_classes)" % who)
        c = FdlpMmodConfigC()
        c.n_streams = M
        for s, cfg in enumerate(self.cfgs[:MAX_STREAMS]):
            c.post[s] = cfg.to_c(device)
        c.in_dim, c.n_sub_layers, c.hidden_sub, c.n_trunk_layers, c.n_classes = (int(v) for v in shape)
        pp = (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays]) if arrays is not None else None
        h = ctypes.c_void_p()
        check(lib.fdlp_mmod_plan_create(ctypes.byref(c), pp, self.max_rows, self.max_utts, ctypes.byref(h)))
        self._h = h
        ind, nt, gu, lds = _lib.c_i32(), _lib.c_i32(), _lib.c_i32(), _lib.c_i32()
        wsb = _lib.c_i64()
        td = (_lib.c_i32 * (_lib.FDLP_RNN_MAX_STAGES + 2))()
        check(lib.fdlp_mmod_plan_info(self._h, ctypes.byref(ind), ctypes.byref(nt), td, ctypes.byref(wsb),
                                      ctypes.byref(gu), ctypes.byref(lds)))
        self.in_dim, self.n_taps = ind.value, nt.value
        self.tap_dims = [td[i] for i in range(nt.value)]
        self.n_sub_layers, self.hidden_sub, self.n_trunk_layers, self.out_dim = (int(shape[1]), int(shape[2]),
                                                                                 int(shape[3]), int(shape[4]))
        self.workspace_bytes, self.group_utts, self.lds_bytes = wsb.value, gu.value, lds.value

    def close(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:   # lib is gone when the interpreter shuts down
            lib.fdlp_mmod_plan_destroy(h)
            self._h = None

    def __del__(self):
        self.close()

    def tap_dim(self, tap: int) -> int:
        if not 0 <= tap < self.n_taps:
            raise ValueError("tap %d is outside 0 .. %d (the model has %d taps)" % (tap, self.n_taps - 1, self.n_taps))
        return self.tap_dims[tap]

    def groups(self, lengths: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, int]:
        """(group_of, slot_of, n_groups) of a batch with these lengths: the one table all streams' scans share"""
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32))
        g, s = np.zeros(lens.size, dtype=np.int32), np.zeros(lens.size, dtype=np.int32)
        n = _lib.c_i32()
        check(lib.fdlp_mmod_plan_groups(self._h, ptr(lens, ctypes.c_int32), lens.size, ptr(g, ctypes.c_int32),
                                        ptr(s, ctypes.c_int32), ctypes.byref(n)))
        return g, s, n.value

    def set_profiling(self, on: bool):
        check(lib.fdlp_mmod_set_profiling(self._h, int(bool(on))))

    def times(self):
        """(ms in the projections and the regression, ms in the scans) since the last call; waits for them"""
        ms = (ctypes.c_double * 2)()
        check(lib.fdlp_mmod_times(self._h, ms))
        return ms[0], ms[1]

    def compute(self, feats: Sequence[torch.Tensor], lengths, norms=None, norm_indexes=None, norm_vars: bool = True,
                tap: int = 0, mode: str = "raw", prior: Optional[torch.Tensor] = None, prior_weight: float = 0.8,
                offsets=None, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """feats[s]: stream s's float32 [rows, cfgs[s].dim] device tensor.  lengths (and offsets): one list for all
        streams, or one list per stream; lists that differ are refused by the library with a message that names the
        utterance.  norms[s], norm_indexes[s]: stream s's norm table as for PostPlan.compute (None: no cmvn there).
        tap, mode, prior, prior_weight, out as for RnnPlan.compute.  Returns out [rows, tap_dim(tap)]."""
        who, M = "MultimodPlan.compute", self.n_streams
        if mode not in MODES:
            raise ValueError("mode must be one of %s" % ", ".join(MODES))
        if len(feats) != M:
            raise ValueError("%s: %d feature tensors for %d streams" % (who, len(feats), M))

        def per_stream(v):
            nested = v is not None and len(v) > 0 and isinstance(v[0], (list, tuple, np.ndarray))
            if nested and len(v) != M:
                raise ValueError("%s: %d lists for %d streams" % (who, len(v), M))
            return list(v) if nested else [v] * M

        lens, offs = per_stream(lengths), per_stream(offsets)
        norms = list(norms) if norms is not None else [None] * M
        idxs = list(norm_indexes) if norm_indexes is not None else [None] * M
        bs, keep = (FdlpPostBatchC * M)(), []
        for s in range(M):
            b, out, k = _make_batch(who, self.cfgs[s].dim, self.tap_dim(tap), feats[s], lens[s], norms[s], idxs[s],
                                    norm_vars, offs[s], out)
            bs[s] = b
            keep.append(k)
        pp = None
        if mode == "loglike":
            if (not isinstance(prior, torch.Tensor) or prior.dtype != torch.float32 or prior.device != feats[0].device
                    or tuple(prior.shape) != (self.out_dim,)):
                raise ValueError("%s: loglike needs prior, a float32 [%d] tensor on the features' device"
                                 % (who, self.out_dim))
            prior = prior.contiguous()
            pp = ctypes.c_void_p(prior.data_ptr())
        st = stream if stream is not None else torch.cuda.current_stream(feats[0].device)
        check(lib.fdlp_mmod_compute(self._h, bs, int(tap), MODES[mode], pp, float(prior_weight),
                                    ctypes.c_void_p(st.cuda_stream)))
        return out


# ---------------------------------------------------------------------------------------------
# the reference's checkpoint: the dict train_multimod_* saves
# ---------------------------------------------------------------------------------------------
@dataclass
class MultimodCheckpoint:
    feature_dim: int
    num_frames: int
    num_classes: int
    mod_num: int
    header: dict
    subnets: List[List[tuple]] = field(default_factory=list)   # [stream][layer] (w_ih, w_hh, b_ih, b_hh)
    trunk: List[tuple] = field(default_factory=list)
    regression: tuple = ()

    num_layers = 0   # NnetRunner's --layer check: only the logits are written


MULTIMOD_KEYS = ("feature_dim", "num_frames", "num_classes", "num_layers_subband", "num_layers", "hidden_dim_subband",
                 "mod_num")


def load_multimod_checkpoint(path: str) -> MultimodCheckpoint:
    """torch.load of the dict the reference's trainer saves: feature_dim, num_frames, num_classes,
    num_layers_subband, num_layers, hidden_dim_subband, mod_num and model_state_dict with
    subnets.{s}.layers.{i}.{weight_ih,weight_hh,bias_ih,bias_hh}_l0, layers.{i}.*_l0 and regression.{weight
    [C, M Hs, 1], bias}.  Every shape is checked against the header; the errors name the key."""
    hdr, sd = open_checkpoint(path, MULTIMOD_KEYS, zero_ok=("num_layers",))
    K0, C = hdr["feature_dim"] * hdr["num_frames"], hdr["num_classes"]
    M, Ls, Hs, Lt = hdr["mod_num"], hdr["num_layers_subband"], hdr["hidden_dim_subband"], hdr["num_layers"]
    if M > MAX_STREAMS:
        raise ValueError("%s: key 'mod_num' is %d; at most %d streams are supported" % (path, M, MAX_STREAMS))
    subnets = [[st[1:] for st in _gru_stages(path, sd, "subnets.%d.layers" % s, Ls, K0, Hs, hdr)] for s in range(M)]
    extra = [k for k in sd.keys() if k.startswith("subnets.") and k.split(".")[1].isdigit() and int(k.split(".")[1]) >= M]
    if extra:
        raise ValueError("%s: model_state_dict has '%s' beyond the mod_num = %d of the header" % (path, extra[0], M))
    trunk = [st[1:] for st in _gru_stages(path, sd, "layers", Lt, M * Hs, M * Hs, hdr)]
    regression = (_state_array(path, sd, "regression.weight", (C, M * Hs), hdr),
                  _state_array(path, sd, "regression.bias", (C,), hdr))
    return MultimodCheckpoint(hdr["feature_dim"], hdr["num_frames"], C, M, hdr, subnets, trunk, regression)


# ---------------------------------------------------------------------------------------------
# runner: RnnRunner's loop on stream 0; one RnnRunner per further stream for what lies before the model
# ---------------------------------------------------------------------------------------------
class MultimodRunner(RnnRunner):
    """The runner IS stream 0's front (its egs.config, its norm, its transform, its table drives the loop); every
    further stream has an RnnRunner of its own for the same things, whose table is read in step.  A slot holds
    stream 0's staging as ever and the other streams' beside it (sl.more)."""
    PROG = "dump-multimod-outputs"

    def __init__(self, ckpt: MultimodCheckpoint, egs: Sequence, **kw):
        if len(egs) != ckpt.mod_num:
            raise ValueError("%d egs.config files for a model of %d streams" % (len(egs), ckpt.mod_num))
        super().__init__(ckpt, egs[0], **kw)
        front = dict(device=self.device, batch_rows=self.batch_rows, log=self.log)
        self.fronts = [self] + [RnnRunner(ckpt, e, **front) for e in egs[1:]]
        self.readers = self.pending = None
        self._cur = None

    # -- the tables ---------------------------------------------------------------------------
    def run(self, rspecifiers: Sequence[str], writer):
        if len(rspecifiers) != len(self.fronts):
            raise ValueError("%d feature tables for a model of %d streams" % (len(rspecifiers), len(self.fronts)))
        self.readers = [None] + [iter(MatReader(r)) for r in rspecifiers[1:]]
        self.pending = [None] + [{} for _ in rspecifiers[1:]]
        return super().run(rspecifiers[0], writer)

    def _reader(self, rspecifier):
        for utt, m in MatReader(rspecifier):
            self._cur = m
            yield utt, m

    def _fetch(self, s, utt):
        """stream s's matrix of utt, or None: the next one of its table, or one passed over before, or one further on"""
        if utt in self.pending[s]:
            return self.pending[s].pop(utt)
        for k, m in self.readers[s]:
            if k == utt:
                return m
            self.pending[s][k] = m.copy()    # the reader's buffer is reused by the next read
        return None

    def _first_dim(self, s):
        for m in self.pending[s].values():
            if m.shape[0] > 0:
                return m.shape[1]
        for k, m in self.readers[s]:
            self.pending[s][k] = m.copy()
            if m.shape[0] > 0:
                return m.shape[1]
        raise ValueError("stream %d has no features" % s)

    # -- SlotRunner's hooks -------------------------------------------------------------------
    def _setup(self, dim):
        for s, f in enumerate(self.fronts[1:], 1):
            f._setup_front(self._first_dim(s))
        super()._setup(dim)

    def _new_plan(self, cfg, rows):
        c = self.ckpt
        cfgs = [PostConfig(dim=c.feature_dim, left_context=f.egs.left, right_context=f.egs.right) for f in self.fronts]
        return MultimodPlan(cfgs, c.subnets, c.trunk, c.regression, max_rows=rows, max_utts=rows, device=self.device)

    def _slot(self, rows):
        sl = super()._slot(rows)
        dev = sl.d_in.device
        sl.more = []
        for f in self.fronts[1:]:
            h_in = torch.empty((rows, f.dim), dtype=torch.float32, pin_memory=True)
            d_in = torch.empty((rows, f.dim), dtype=torch.float32, device=dev)
            d_mid = (torch.empty((rows, self.ckpt.feature_dim), dtype=torch.float32, device=dev)
                     if f.pre is not None else None)
            sl.more.append((h_in, d_in, d_mid))
        return sl

    def _admit(self, utt):
        T = self._cur.shape[0]
        mats = [self._fetch(s, utt) for s in range(1, len(self.fronts))]   # every table moves on, admitted or not
        for s, m in enumerate(mats, 1):
            if m is None:
                self.log("utterance %s is missing from stream %d, producing no output for it" % (utt, s))
                self.num_err += 1
                return False
            if m.shape[0] != T or m.shape[1] != self.fronts[s].dim:
                self.log("utterance %s has %d x %d features in stream %d and %d frames in stream 0, producing no "
                         "output for it" % (utt, m.shape[0], m.shape[1], s, T))
                self.num_err += 1
                return False
        extras = [super()._admit(utt)]
        if extras[0] is False:
            return False
        for f in self.fronts[1:]:
            e = RnnRunner._admit(f, utt)       # logs; the count is kept here
            if e is False:
                self.num_err += 1
                return False
            extras.append(e)
        return mats, extras

    def _added(self, sl, extra):
        mats, extras = extra
        T = sl.lens[-1]
        for (h_in, _, _), m in zip(sl.more, mats):
            h_in[sl.fill - T:sl.fill].numpy()[...] = m
        sl.norms.append(extras)     # per stream: None, or the utterance's own norm

    def _launch(self, sl):
        n = sl.fill
        feats, norms, idxs = [], [], []
        bufs = [(sl.h_in, sl.d_in, sl.d_mid)] + sl.more
        for s, (f, (h_in, d_in, d_mid)) in enumerate(zip(self.fronts, bufs)):
            d = d_in[:n]
            d.copy_(h_in[:n], non_blocking=True)
            if f.pre is not None:
                d = f.pre.compute(d, sl.lens, f.pca, out=d_mid)[:n]
            feats.append(d)
            if f.utt_stats is None:
                norms.append(f.norm)
                idxs.append(None)
            else:
                norms.append(torch.from_numpy(np.stack([e[s] for e in sl.norms])).to(d.device))
                idxs.append(list(range(len(sl.norms))))
        self.plan.compute(feats, sl.lens, norms=norms, norm_indexes=idxs, norm_vars=self.NORM_VARS, tap=0,
                          mode=self.mode, prior=self.prior, prior_weight=self.prior_weight, out=sl.d_out)
        sl.h_out[:n].copy_(sl.d_out[:n], non_blocking=True)
        sl.done = torch.cuda.Event()
        sl.done.record()


# ---------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------
def dump_multimod_outputs_parser():
    ap = argparse.ArgumentParser(prog="dump-multimod-outputs",
                                 description="Logits, posteriors or pseudo log-likelihoods of a multi-stream GRU "
                                             "acoustic model, on the MI355X")
    ap.add_argument("model", help="checkpoint of the multi-stream model, as the reference's trainer saves it")
    ap.add_argument("scps", help="feats.scp of every stream, separated by commas (or ark: / scp: rspecifiers)")
    ap.add_argument("egs_configs", help="the egs.config pickle of every stream, separated by commas")
    ap.add_argument("save_file", help="output base name: <save_file>.ark and .scp are written (or an ark wspecifier)")
    ap.add_argument("--prior", default=None, help="pickle of the log prior [num_classes]: write log_softmax - prior_weight * prior")
    ap.add_argument("--prior_weight", type=float, default=0.8, help="weight of the prior (default 0.8)")
    ap.add_argument("--add_softmax", action="store_true", help="write softmax posteriors instead of logits (ignored with --prior)")
    ap.add_argument("--override_trans", default=None, help="accepted and ignored, as in the reference")
    ap.add_argument("--ark_precision", type=int, default=3, help="decimals of the written values, like the "
                    "reference's '%%.3f' text ark; negative keeps float32")
    ap.add_argument("--device", type=int, default=int(os.environ.get("FDLP_DEVICE", "0")))
    ap.add_argument("--batch-rows", type=int, default=131072, help="rows per device batch (whole utterances)")
    return ap


def main_dump_multimod_outputs(argv=None):
    prog = "dump-multimod-outputs"
    a = dump_multimod_outputs_parser().parse_args(argv)
    if a.override_trans is not None:
        print("WARNING (%s) --override_trans is ignored, as in the reference" % prog, file=sys.stderr)
    scps, egs_paths = a.scps.split(","), a.egs_configs.split(",")
    try:
        ckpt = load_multimod_checkpoint(a.model)
    except (OSError, ValueError) as e:
        print("ERROR (%s) %s" % (prog, e), file=sys.stderr)
        return 1
    if len(egs_paths) != ckpt.mod_num:
        print("ERROR (%s) Modulation numbers not matching number of egs.config files given!" % prog, file=sys.stderr)
        return 1
    if len(scps) != ckpt.mod_num:
        print("ERROR (%s) Number of modulations does not match with number of scp files given!" % prog, file=sys.stderr)
        return 1

    def make_runner():
        egs = [load_rnn_egs_config(p) for p in egs_paths]
        mode, prior = "raw", None
        if a.prior:
            mode, prior = "loglike", _load_prior(a.prior)
        elif a.add_softmax:
            mode = "softmax"
        return MultimodRunner(ckpt, egs, mode=mode, prior=prior, prior_weight=a.prior_weight, device=a.device,
                              batch_rows=a.batch_rows, decimals=a.ark_precision, prog=prog)

    return run_model_tool(prog, a, make_runner, "Dumped outputs", scps=scps)


if __name__ == "__main__":
    sys.exit(main_dump_multimod_outputs(sys.argv[1:]))
