// fdlp_plan_model.cpp -- the acoustic-model plans behind the chain (fdlp_plan_post.cpp): the stage plan with its
// rnn and nnet fronts, and the multi-stream plan.
#include <string.h>

#include "fdlp_plan_common.h"

using fdlp::fail;
using namespace fdlp::host;

// ---------------------------------------------------------------------------------------------
// Stage plan (cmvn | deltas | splice | a list of GRU and linear stages): a transform plan for stage 0 (a linear
// stage's [W | b] or a GRU's [W_ih | b_ih]), the other weights on the device, the G buffer of the input projections,
// two workspaces the stages ping-pong between, and the group table of gru_scan_kernel.  fdlp_rnn_* is its public
// face; fdlp_nnet_* (below it) is the same plan with the stages linear_relu x (n_linear - 1), linear and no scans.
// ---------------------------------------------------------------------------------------------
// what a front calls itself and its parts in the messages
struct StageWords {
  const char *create, *compute, *model, *stage;
};
static const StageWords kRnnWords = {"fdlp_rnn_plan_create", "fdlp_rnn_compute", "model", "stage"};
static const StageWords kNnetWords = {"fdlp_nnet_plan_create", "fdlp_nnet_compute", "network", "layer"};
static const StageWords kVencWords = {"fdlp_venc_create", "fdlp_venc_compute", "model", "stage"};

// Stage kinds beside the public FDLP_RNN_*: only the venc front (at the bottom) makes them, with a ConvGeom.
//   kStageConv  a same-padded Conv2d over rows [t][c F + f] (conv2d_same_kernel), {w [Co, Ci, kh, kw], -, b, -};
//               dims[s] = Ci F, dims[s + 1] = Co F; its ReLU is applied when the next stage loads the output
//   kStageNorm  the per-utterance normaliser (utt_norm_kernel), no parameters, dims[s + 1] = dims[s]
// A plan whose stage 0 is a conv runs the plain chain (post_kernel) in front of it instead of a fused transform.
enum { kStageConv = 3, kStageNorm = 4 };
struct ConvGeom {
  int F, kh, kw;
};

// Utterances sorted by length, descending and stable, cut into groups of kGruGU: order[i] is the utterance in
// slot i % kGruGU of group i / kGruGU
static std::vector<int> rnn_group_order(const int64_t* len, int n) {
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });
  return order;
}

// The group table of gru_scan_kernel on the device and its pinned staging copy: what every plan with a scan owns
// (the stage plan, the multi-stream plan).  The owner's device is current in every call.
struct GroupTable {
  int max_groups = 0;
  Staging<fdlp::GruSlot> slots;

  int64_t bytes() const { return (int64_t)sizeof(fdlp::GruSlot) * max_groups * fdlp::kGruGU; }
  int alloc(DeviceResources& res) {
    if (max_groups <= 0) return FDLP_OK;
    if (slots.arrays(res, (size_t)max_groups * fdlp::kGruGU) != hipSuccess)
      return fail(FDLP_E_NOMEM, "stage plan: group table allocation failed");
    if (slots.event(res) != hipSuccess) return fail(FDLP_E_NOMEM, "stage plan: event creation failed");
    return FDLP_OK;
  }
  // the table of batch b, once per batch: *ng groups, copied on stream s
  int stage(const fdlp_post_batch* b, hipStream_t s, int* ng) {
    *ng = (b->n_utt + fdlp::kGruGU - 1) / fdlp::kGruGU;
    int rc;
    if ((rc = slots.wait()) != FDLP_OK) return rc;
    const std::vector<int> order = rnn_group_order(b->utt_len, b->n_utt);
    for (int i = 0; i < *ng * fdlp::kGruGU; ++i) {
      fdlp::GruSlot& sl = slots.host[i];
      sl.row0 = i < b->n_utt ? b->row_off[order[(size_t)i]] : 0;
      sl.len = i < b->n_utt ? (int32_t)b->utt_len[order[(size_t)i]] : 0;
      sl.pad = 0;
    }
    return slots.publish((size_t)*ng * fdlp::kGruGU, s);
  }
};

// HIP events around every launch of a compute while profiling is on, summed per class by times()
struct LaunchMarks {
  bool profile = false;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> marks;  // (0 projection | 1 scan, start, stop)
  hipEvent_t ev0 = nullptr;

  ~LaunchMarks() { drop(); }
  hipError_t begin(hipStream_t s) {
    if (!profile) return hipSuccess;
    hipError_t e = hipEventCreate(&ev0);
    return e != hipSuccess ? e : hipEventRecord(ev0, s);
  }
  hipError_t end(int cls, hipStream_t s) {
    if (!profile) return hipSuccess;
    hipEvent_t ev1 = nullptr;
    hipError_t e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev1, s);
    marks.push_back({cls, {ev0, ev1}});
    return e;
  }
  void drop() {
    for (auto& m : marks) {
      (void)hipEventDestroy(m.second.first);
      (void)hipEventDestroy(m.second.second);
    }
    marks.clear();
  }
  // ms[0] the projections and linear stages, ms[1] the scans, ms[2] (n = 3: the venc front) the convolutions since
  // the last call; waits for them
  int times(double* ms, int n = 2) {
    for (int i = 0; i < n; ++i) ms[i] = 0.0;
    for (auto& m : marks) {
      float t = 0.f;
      HIP_TRY(hipEventSynchronize(m.second.second));
      HIP_TRY(hipEventElapsedTime(&t, m.second.first, m.second.second));
      ms[std::min(m.first, n - 1)] += t;
    }
    drop();
    return FDLP_OK;
  }
};

struct fdlp_rnn_plan {
  const StageWords* words = &kRnnWords;
  std::unique_ptr<fdlp_xform_plan> l0;
  int n_stages = 0, device = -1;
  std::vector<int> kind, dims;  // n_stages, n_stages + 1
  int64_t max_rows = 0;
  int max_utts = 0;             // 0 behind the nnet front (as gt.max_groups): no scans, no group table, any n_utt
  int max_h = 0;                // widest GRU, 0 without one
  int widest = 0;               // widest of dims[1 .. n_stages - 1] (with a conv stage 0, which reads a workspace,
                                // of dims[0 .. n_stages - 1]), 0 with one stage
  float* d_m0 = nullptr;        // [N_0, dims[0] + 1], N_0 = dims[1] or 3 dims[1]
  std::vector<float*> d_p;      // 4 per stage: w_ih | w, w_hh, b_ih | b, b_hh (stage 0: w_hh and b_hh only)
  float* d_g = nullptr;
  float* d_ws[2] = {nullptr, nullptr};
  GroupTable gt;
  LaunchMarks lm;
  // conv stages (the venc front with a CNN encoder): the image height and the kernel, the plain chain in front of
  // a conv stage 0, a koff table per conv stage, the tile table of a batch (one for all layers: it depends on F alone)
  ConvGeom cg{0, 0, 0};
  std::unique_ptr<fdlp_post_plan> c0;
  std::vector<int32_t*> d_koff;
  Staging<fdlp::ConvTile> ctiles;
  size_t conv_lds = 0;
  DeviceResources res;
};

// n zeroed float32 on the device: rows no utterance covers are read by the dense launches (and never stored into
// an utterance's rows)
static int zeroed_workspace(DeviceResources& res, float** ws, size_t n, const char* what, int64_t max_rows) {
  if (n == 0) return FDLP_OK;
  if (res.device_array(ws, n) != hipSuccess) {
    *ws = nullptr;
    return fail(FDLP_E_NOMEM, std::string("stage plan: allocation of ") + what + " failed: " + std::to_string(n) +
                                  " float32 for " + std::to_string(max_rows) + " rows");
  }
  if (hipMemset(*ws, 0, sizeof(float) * n) != hipSuccess) return fail(FDLP_E_HIP, "stage plan: memset failed");
  return FDLP_OK;
}

// max_utts = 0 (the nnet front; legal without a GRU only): no scans, so no group table, staging or event
// cg: the geometry of the conv stages; without it only the public kinds are known
static int stage_plan_create(const fdlp_rnn_config* cfg, const float* const* params, int64_t max_rows,
                             int32_t max_utts, const StageWords& w, fdlp_rnn_plan** out,
                             const ConvGeom* cg = nullptr) {
  *out = nullptr;
  const int ns = cfg->n_stages;
  if (ns < 1 || ns > FDLP_RNN_MAX_STAGES)
    return fail(FDLP_E_INVALID, "the model needs 1 .. " + std::to_string(FDLP_RNN_MAX_STAGES) +
                                    " stages, got n_stages = " + std::to_string(ns));
  std::string shape;
  for (int s = 0; s <= ns; ++s) shape += (s ? " -> " : "") + std::to_string(cfg->dims[s]);
  for (int s = 0; s < ns; ++s)
    if (cfg->kind[s] != FDLP_RNN_GRU && cfg->kind[s] != FDLP_RNN_LINEAR && cfg->kind[s] != FDLP_RNN_LINEAR_RELU &&
        !(cg && (cfg->kind[s] == kStageConv || (cfg->kind[s] == kStageNorm && s > 0))))
      return fail(FDLP_E_INVALID, "stage " + std::to_string(s) + " has the unknown kind " +
                                      std::to_string(cfg->kind[s]) + " (0 GRU, 1 linear, 2 linear with ReLU)");
  for (int s = 0; s <= ns; ++s)
    if (cfg->dims[s] < 1)
      return fail(FDLP_E_INVALID, std::string(w.model) + " dimension " + std::to_string(s) + " is " +
                                      std::to_string(cfg->dims[s]) + " (every dimension must be >= 1; dims " + shape +
                                      ")");
  if (max_rows < 1) return fail(FDLP_E_INVALID, "max_rows must be >= 1, got " + std::to_string(max_rows));
  int max_h = 0;
  for (int s = 0; s < ns; ++s)
    if (cfg->kind[s] == FDLP_RNN_GRU) max_h = std::max(max_h, cfg->dims[s + 1]);
  if (max_utts < (max_h > 0 ? 1 : 0))
    return fail(FDLP_E_INVALID, "max_utts must be >= 1, got " + std::to_string(max_utts));
  if (max_h > fdlp::gru_max_hidden())
    return fail(FDLP_E_INVALID, "a GRU of " + std::to_string(max_h) + " hidden units needs " +
                                    std::to_string(fdlp::gru_lds_bytes(max_h)) + " bytes of the 163840-byte LDS; the "
                                    "widest that fits has " + std::to_string(fdlp::gru_max_hidden()));
  size_t conv_lds = 0;
  for (int s = 0; s < ns; ++s) {
    if (cfg->kind[s] == kStageNorm && cfg->dims[s + 1] != cfg->dims[s])
      return fail(FDLP_E_INVALID, "stage " + std::to_string(s) + " normalises " + std::to_string(cfg->dims[s]) +
                                      " columns into " + std::to_string(cfg->dims[s + 1]));
    if (cfg->kind[s] != kStageConv) continue;
    const int F = cg->F, Ci = cfg->dims[s] / std::max(F, 1), Co = cfg->dims[s + 1] / std::max(F, 1);
    if (F < 1 || cg->kh < 1 || cg->kw < 1 || cg->kh % 2 == 0 || cg->kw % 2 == 0)
      return fail(FDLP_E_INVALID, "a same-padded convolution needs an odd kernel and a height >= 1, got kernel (" +
                                      std::to_string(cg->kh) + ", " + std::to_string(cg->kw) + ") at height " +
                                      std::to_string(F));
    if (Ci * F != cfg->dims[s] || Co * F != cfg->dims[s + 1])
      return fail(FDLP_E_INVALID, "stage " + std::to_string(s) + " is a convolution at height " + std::to_string(F) +
                                      " from " + std::to_string(cfg->dims[s]) + " to " +
                                      std::to_string(cfg->dims[s + 1]) + " columns, which are not whole channels");
    const int64_t K = (int64_t)Ci * cg->kh * cg->kw;
    const double need = K > (1 << 24) ? 4.0 * (double)K : (double)fdlp::conv_lds_bytes(F, Ci, Co, cg->kh, cg->kw);
    if (need > 163840.0)
      return fail(FDLP_E_INVALID, "the convolution of stage " + std::to_string(s) + ", " + std::to_string(Ci) +
                                      " -> " + std::to_string(Co) + " channels, kernel (" + std::to_string(cg->kh) +
                                      ", " + std::to_string(cg->kw) + ") at height " + std::to_string(F) +
                                      ", needs " + std::to_string((long long)need) +
                                      " bytes of the 163840-byte LDS (the staged input patch holds " +
                                      std::to_string(fdlp::conv_patch_frames(F, cg->kw)) + " frames of " +
                                      std::to_string((int64_t)Ci * (F + cg->kh - 1)) + " floats)");
    conv_lds = std::max(conv_lds, (size_t)need);
  }
  const bool conv0 = cfg->kind[0] == kStageConv;
  const bool dev = cfg->post.device >= 0;
  if (dev && !params) return fail(FDLP_E_INVALID, std::string(w.create) + ": null parameters");
  for (int s = 0; dev && s < ns; ++s) {
    const bool gru = cfg->kind[s] == FDLP_RNN_GRU;
    if (cfg->kind[s] == kStageNorm) continue;
    if (!params[4 * s] || !params[4 * s + 2] || (gru && (!params[4 * s + 1] || !params[4 * s + 3])))
      return fail(FDLP_E_INVALID, std::string(w.create) + ": null parameters of " + w.stage + " " + std::to_string(s));
  }
  PlanPtr<fdlp_rnn_plan> p(new (std::nothrow) fdlp_rnn_plan);
  if (!p) return fail(FDLP_E_NOMEM, "out of memory");
  p->words = &w;
  p->n_stages = ns;
  p->device = p->res.device = cfg->post.device;
  p->kind.assign(cfg->kind, cfg->kind + ns);
  p->dims.assign(cfg->dims, cfg->dims + ns + 1);
  p->max_rows = max_rows;
  p->max_utts = max_utts;
  p->gt.max_groups = (max_utts + fdlp::kGruGU - 1) / fdlp::kGruGU;
  p->max_h = max_h;
  for (int s = conv0 ? 0 : 1; s < ns; ++s) p->widest = std::max(p->widest, cfg->dims[s]);  // a conv stage 0 reads a workspace
  p->d_p.assign((size_t)ns * 4, nullptr);
  p->d_koff.assign((size_t)ns, nullptr);
  if (cg) p->cg = *cg;
  p->conv_lds = conv_lds;
  int rc;
  const int N0 = cfg->kind[0] == FDLP_RNN_GRU ? 3 * cfg->dims[1] : cfg->dims[1];
  if (conv0) {
    fdlp_post_plan* c0 = nullptr;
    if ((rc = fdlp_post_plan_create(&cfg->post, &c0)) != FDLP_OK) return rc;
    p->c0.reset(c0);
  } else {
    fdlp_xform_config xc{};
    xc.post = cfg->post;
    xc.out_dim = N0;
    xc.affine = 1;
    fdlp_xform_plan* l0 = nullptr;
    if ((rc = fdlp_xform_plan_create(&xc, &l0)) != FDLP_OK) return rc;
    p->l0.reset(l0);
  }
  const int K0 = conv0 ? p->c0->Dout : p->l0->post->Dout;
  if (K0 != cfg->dims[0])
    return fail(FDLP_E_INVALID, std::string("the ") + w.model + "'s input dimension dims[0] = " +
                                    std::to_string(cfg->dims[0]) + " differs from the " + std::to_string(K0) +
                                    " columns the stages before it give");
  if (!dev) {
    *out = p.release();
    return FDLP_OK;
  }
  DeviceGuard dg(p->device);
  if (dg.status() != hipSuccess) return fail(FDLP_E_HIP, "hipSetDevice failed");
  DeviceResources& res = p->res;
  if (!conv0) {
    // stage 0's input side as transform-feats' affine matrix: [W | b]
    std::vector<float> m0((size_t)N0 * (K0 + 1));
    for (int n = 0; n < N0; ++n) {
      memcpy(&m0[(size_t)n * (K0 + 1)], params[0] + (size_t)n * K0, sizeof(float) * K0);
      m0[(size_t)n * (K0 + 1) + K0] = params[2][n];
    }
    if ((rc = upload(res, &p->d_m0, m0.data(), m0.size())) != FDLP_OK) return rc;
  }
  for (int s = 0; s < ns; ++s) {
    const size_t K = (size_t)cfg->dims[s], N = (size_t)cfg->dims[s + 1];
    const bool gru = cfg->kind[s] == FDLP_RNN_GRU;
    if (cfg->kind[s] == kStageNorm) continue;
    if (cfg->kind[s] == kStageConv) {
      // w [Co, Ci kh kw], b [Co], and the offsets of the k into the staged patch
      const size_t F = (size_t)cg->F, Ci = K / F, Co = N / F, Kc = Ci * cg->kh * cg->kw;
      if ((rc = upload(res, &p->d_p[4 * (size_t)s], params[4 * s], Co * Kc)) != FDLP_OK ||
          (rc = upload(res, &p->d_p[4 * (size_t)s + 2], params[4 * s + 2], Co)) != FDLP_OK)
        return rc;
      std::vector<int32_t> koff((Kc + fdlp::kDenseKC - 1) / fdlp::kDenseKC * fdlp::kDenseKC);
      fdlp::conv_koff_table((int)F, (int)Ci, cg->kh, cg->kw, koff.data());
      if ((rc = upload(res, &p->d_koff[(size_t)s], koff.data(), koff.size())) != FDLP_OK) return rc;
      continue;
    }
    // w_ih | w, w_hh, b_ih | b, b_hh; stage 0's input side is d_m0
    const size_t count[4] = {s > 0 ? (gru ? 3 * N : N) * K : 0, gru ? 3 * N * N : 0, s > 0 ? (gru ? 3 * N : N) : 0,
                             gru ? 3 * N : 0};
    for (int i : {0, 2, 1, 3})  // the input side first
      if (count[i] && (rc = upload(res, &p->d_p[4 * (size_t)s + i], params[4 * s + i], count[i])) != FDLP_OK) return rc;
  }
  if (conv_lds && p->ctiles.event(res) != hipSuccess) return fail(FDLP_E_NOMEM, "stage plan: event creation failed");
  if ((rc = zeroed_workspace(res, &p->d_g, (size_t)max_rows * 3 * p->max_h, "the projection buffer", max_rows)) != FDLP_OK)
    return rc;
  for (float*& ws : p->d_ws)
    if ((rc = zeroed_workspace(res, &ws, (size_t)max_rows * p->widest, "a stage workspace", max_rows)) != FDLP_OK) return rc;
  if ((rc = p->gt.alloc(res)) != FDLP_OK) return rc;
  *out = p.release();
  return FDLP_OK;
}

// in_dim, the number of stages, their widths and the workspace bytes: what both fronts' info calls share
static void stage_plan_sizes(const fdlp_rnn_plan* p, int32_t* in_dim, int32_t* n_stages, int32_t* out_dims,
                             int64_t* workspace_bytes) {
  if (in_dim) *in_dim = p->dims[0];
  if (n_stages) *n_stages = p->n_stages;
  if (out_dims)
    for (int s = 0; s < p->n_stages; ++s) out_dims[s] = p->dims[(size_t)s + 1];
  if (workspace_bytes)
    *workspace_bytes = (int64_t)sizeof(float) * p->max_rows * (3 * (int64_t)p->max_h + 2 * (int64_t)p->widest) +
                       p->gt.bytes();
}

// fdlp_rnn_plan_groups and fdlp_mmod_plan_groups: the table of a batch with these lengths, on the host
static int group_table_of(const char* who, const int32_t* lengths, int32_t n_utts, int32_t* group_of, int32_t* slot_of,
                          int32_t* n_groups) {
  if (n_utts < 0 || (n_utts > 0 && !lengths)) return fail(FDLP_E_INVALID, std::string(who) + ": bad arguments");
  std::vector<int64_t> len((size_t)n_utts);
  for (int u = 0; u < n_utts; ++u) {
    if (lengths[u] < 1)
      return fail(FDLP_E_INVALID, "utterance " + std::to_string(u) + " has length " + std::to_string(lengths[u]) +
                                      " (every length must be >= 1)");
    len[(size_t)u] = lengths[u];
  }
  const std::vector<int> order = rnn_group_order(len.data(), n_utts);
  for (int i = 0; i < n_utts; ++i) {
    if (group_of) group_of[order[(size_t)i]] = i / fdlp::kGruGU;
    if (slot_of) slot_of[order[(size_t)i]] = i % fdlp::kGruGU;
  }
  if (n_groups) *n_groups = (n_utts + fdlp::kGruGU - 1) / fdlp::kGruGU;
  return FDLP_OK;
}

int fdlp_rnn_plan_create(const fdlp_rnn_config* cfg, const float* const* params, int64_t max_rows, int32_t max_utts,
                         fdlp_rnn_plan** out) {
  if (!cfg || !out) return fail(FDLP_E_INVALID, "fdlp_rnn_plan_create: null argument");
  *out = nullptr;
  if (max_utts < 1) return fail(FDLP_E_INVALID, "max_utts must be >= 1, got " + std::to_string(max_utts));
  return stage_plan_create(cfg, params, max_rows, max_utts, kRnnWords, out);
}

int fdlp_rnn_plan_destroy(fdlp_rnn_plan* p) { delete p; return FDLP_OK; }

int fdlp_rnn_plan_info(const fdlp_rnn_plan* p, int32_t* in_dim, int32_t* n_stages, int32_t* out_dims,
                       int64_t* workspace_bytes, int32_t* group_utts, int32_t* lds_bytes) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_rnn_plan_info: null plan");
  stage_plan_sizes(p, in_dim, n_stages, out_dims, workspace_bytes);
  if (group_utts) *group_utts = fdlp::kGruGU;
  if (lds_bytes) *lds_bytes = p->max_h ? (int32_t)fdlp::gru_lds_bytes(p->max_h) : 0;
  return FDLP_OK;
}

int fdlp_rnn_plan_groups(const fdlp_rnn_plan* p, const int32_t* lengths, int32_t n_utts, int32_t* group_of,
                         int32_t* slot_of, int32_t* n_groups) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_rnn_plan_groups: bad arguments");
  return group_table_of("fdlp_rnn_plan_groups", lengths, n_utts, group_of, slot_of, n_groups);
}

int fdlp_rnn_set_profiling(fdlp_rnn_plan* p, int32_t on) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_rnn_set_profiling: null plan");
  p->lm.profile = on != 0;
  return FDLP_OK;
}

int fdlp_rnn_times(fdlp_rnn_plan* p, double* ms) {
  if (!p || !ms) return fail(FDLP_E_INVALID, "fdlp_rnn_times: null argument");
  DeviceGuard dg(p->device);
  return p->lm.times(ms);
}

// What a compute call asks for, checked before anything is launched: the tap among n_taps, the mode, the prior,
// and the batch against the plan's limits.  `scanned`: the plan has a GRU, whose scans index G and the stage
// outputs through the group table, so every utterance must lie inside the batch's rows (a plan without one leaves
// its batch to the chain's checks alone).
static int stage_check_call(const StageWords& words, int n_taps, int32_t tap, int32_t mode, const void* prior_dev,
                            const fdlp_post_batch* b, int max_utts, int64_t max_rows, bool scanned) {
  auto who = [&](const char* what) { return std::string(words.compute) + ": " + what; };  // built on refusal only
  if (tap < 0 || tap >= n_taps)
    return fail(FDLP_E_INVALID, "tap " + std::to_string(tap) + " is outside 0 .. " + std::to_string(n_taps - 1) +
                                    " (the " + words.model + " has " + std::to_string(n_taps) + " " +
                                    words.stage + "s)");
  if (mode != FDLP_NNET_RAW && mode != FDLP_NNET_SOFTMAX && mode != FDLP_NNET_LOGLIKE)
    return fail(FDLP_E_INVALID, who("unknown mode ") + std::to_string(mode));
  if (mode != FDLP_NNET_RAW && tap != 0)
    return fail(FDLP_E_INVALID, std::string("softmax and loglike apply to the last ") + words.stage +
                                    " only (tap 0), got tap " + std::to_string(tap));
  if (mode == FDLP_NNET_LOGLIKE && (!prior_dev || ((uintptr_t)prior_dev & 3u)))
    return fail(FDLP_E_INVALID, "loglike needs a 4-byte aligned device prior vector");
  if (max_utts > 0 && b->n_utt > max_utts)
    return fail(FDLP_E_INVALID, "batch of " + std::to_string(b->n_utt) + " utterances exceeds the plan's max_utts " +
                                    std::to_string(max_utts));
  if (b->n_rows > max_rows)
    return fail(FDLP_E_CAPACITY, "batch of " + std::to_string(b->n_rows) + " rows exceeds the plan's max_rows " +
                                     std::to_string(max_rows));
  if (b->n_utt > 0 && (!b->out_dev || ((uintptr_t)b->out_dev & 3u)))
    return fail(FDLP_E_INVALID, who("out_dev must be a 4-byte aligned device pointer"));
  const int n_scanned = scanned ? b->n_utt : 0;
  if (n_scanned > 0 && (!b->row_off || !b->utt_len)) return fail(FDLP_E_INVALID, who("bad batch"));
  for (int u = 0; u < n_scanned; ++u) {
    const int64_t T = b->utt_len[u], r0 = b->row_off[u];
    if (T < 1 || T > max_rows || T > INT32_MAX || r0 < 0 || r0 > b->n_rows - T)
      return fail(FDLP_E_INVALID, "utterance " + std::to_string(u) + " has length " + std::to_string(T) +
                                      " at row " + std::to_string(r0) + " of a batch of " +
                                      std::to_string(b->n_rows) + " rows (every length must be >= 1 and inside it)");
  }
  return FDLP_OK;
}

// One stage after the first, marked for the profile: the input projection (or the whole linear stage) of `in`
// [rows, K] in dense_kernel, then for a GRU the one-stream scan of d_g into `out`.  w: the stage's four device arrays.
static int stage_launch(LaunchMarks& lm, bool gru, const float* in, int relu, const float* const* w, float* d_g,
                        float* out, const fdlp::GruSlot* d_slots, int ng, int64_t rows, int K, int N, hipStream_t s) {
  HIP_TRY(lm.begin(s));
  HIP_TRY(fdlp::launch_dense(in, w[0], w[2], gru ? d_g : out, rows, K, gru ? 3 * N : N, relu, s));
  HIP_TRY(lm.end(0, s));
  if (gru) {
    HIP_TRY(lm.begin(s));
    HIP_TRY(fdlp::launch_gru_scan(d_g, w[1], w[3], out, d_slots, ng, rows, N, s));
    HIP_TRY(lm.end(1, s));
  }
  return FDLP_OK;
}

static int stage_compute(fdlp_rnn_plan* p, const fdlp_post_batch* b, int32_t tap, int32_t mode, const void* prior_dev,
                         float prior_weight, void* stream) {
  const StageWords& words = *p->words;
  if (p->device < 0) return fail(FDLP_E_INVALID, std::string(words.compute) + ": host-only plan");
  {
    const int rc = stage_check_call(words, p->n_stages, tap, mode, prior_dev, b, p->max_utts, p->max_rows,
                                    p->max_h > 0 || p->conv_lds > 0);
    if (rc != FDLP_OK) return rc;
  }
  const int last = p->n_stages - 1 - tap;  // the tapped stage
  hipStream_t s = (hipStream_t)stream;
  auto gru = [&](int st) { return p->kind[(size_t)st] == FDLP_RNN_GRU; };
  // where stage st's output goes, and where its input comes from
  auto dst = [&](int st) { return st == last ? (float*)b->out_dev : p->d_ws[st & 1]; };
  DeviceGuard dg(p->device);
  HIP_TRY(dg.status());
  LaunchMarks& lm = p->lm;
  auto kind = [&](int st) { return p->kind[(size_t)st]; };
  const bool conv0 = kind(0) == kStageConv;
  // stage 0's input side in the chain's launch (a conv stage 0: the plain chain into the workspace it reads); its
  // batch checks are the chain's
  fdlp_post_batch b0 = *b;
  b0.out_dev = conv0 ? p->d_ws[1] : gru(0) ? p->d_g : dst(0);
  fdlp::XformConsts xc{};
  xc.N = gru(0) ? 3 * p->dims[1] : p->dims[1]; xc.C = p->dims[0] + 1; xc.affine = 1; xc.n_mat = 1;
  HIP_TRY(lm.begin(s));
  {
    const int rc = conv0 ? post_compute(p->c0.get(), &b0, stream, nullptr, nullptr, nullptr)
                         : post_compute(p->l0->post.get(), &b0, stream, &xc, p->d_m0, nullptr);
    if (rc != FDLP_OK) return rc;
  }
  HIP_TRY(lm.end(0, s));
  if (b->n_utt == 0 || b->n_rows == 0) return FDLP_OK;
  int ng = 0;
  if (p->max_h > 0) {
    const int rc = p->gt.stage(b, s, &ng);
    if (rc != FDLP_OK) return rc;
  }
  // the conv tiles of the batch, once for all conv stages: kDenseTM positions p = t F + f of one utterance each
  size_t nct = 0;
  if (p->conv_lds) {
    const int F = p->cg.F;
    for (int u = 0; u < b->n_utt; ++u) {
      if (b->utt_len[u] > INT32_MAX / F)
        return fail(FDLP_E_CAPACITY, "utterance " + std::to_string(u) + " has " + std::to_string(b->utt_len[u]) +
                                         " frames of height " + std::to_string(F) + ": more than 2^31 - 1 positions");
      nct += (size_t)((b->utt_len[u] * F + fdlp::kDenseTM - 1) / fdlp::kDenseTM);
    }
    if (nct > (size_t)INT32_MAX) return fail(FDLP_E_CAPACITY, "too many convolution tiles in one batch");
    int rc;
    if ((rc = p->ctiles.wait()) != FDLP_OK) return rc;
    if ((rc = p->ctiles.reserve(p->res, nct, "stage plan: convolution tile table allocation failed")) != FDLP_OK) return rc;
    size_t k = 0;
    for (int u = 0; u < b->n_utt; ++u)
      for (int64_t p0 = 0; p0 < b->utt_len[u] * F; p0 += fdlp::kDenseTM) {
        fdlp::ConvTile& tl = p->ctiles.host[k++];
        tl.row0 = b->row_off[u];
        tl.T = (int32_t)b->utt_len[u];
        tl.p0 = (int32_t)p0;
      }
    if ((rc = p->ctiles.publish(nct, s)) != FDLP_OK) return rc;
  }
  auto conv = [&](int st, const float* in, int relu) -> int {
    const int F = p->cg.F;
    HIP_TRY(lm.begin(s));
    HIP_TRY(fdlp::launch_conv2d_same(in, p->d_p[4 * (size_t)st], p->d_p[4 * (size_t)st + 2], dst(st), p->ctiles.dev,
                                     (int)nct, p->d_koff[(size_t)st], b->n_rows, F, p->dims[(size_t)st] / F,
                                     p->dims[(size_t)st + 1] / F, p->cg.kh, p->cg.kw, relu, s));
    HIP_TRY(lm.end(2, s));
    return FDLP_OK;
  };
  if (conv0) {
    const int rc = conv(0, p->d_ws[1], 0);
    if (rc != FDLP_OK) return rc;
  }
  if (gru(0)) {
    const float* const* w = &p->d_p[0];
    HIP_TRY(lm.begin(s));
    HIP_TRY(fdlp::launch_gru_scan(p->d_g, w[1], w[3], dst(0), p->gt.slots.dev, ng, b->n_rows, p->dims[1], s));
    HIP_TRY(lm.end(1, s));
  }
  for (int st = 1; st <= last; ++st) {
    const int relu = kind(st - 1) == FDLP_RNN_LINEAR_RELU || kind(st - 1) == kStageConv;
    if (kind(st) == kStageConv) {
      const int rc = conv(st, p->d_ws[(st - 1) & 1], relu);
      if (rc != FDLP_OK) return rc;
      continue;
    }
    if (kind(st) == kStageNorm) {
      HIP_TRY(lm.begin(s));
      HIP_TRY(fdlp::launch_utt_norm(p->d_ws[(st - 1) & 1], dst(st), p->gt.slots.dev, ng * fdlp::kGruGU, b->n_rows,
                                    p->dims[(size_t)st], s));
      HIP_TRY(lm.end(0, s));
      continue;
    }
    const int rc = stage_launch(lm, gru(st), p->d_ws[(st - 1) & 1], relu, &p->d_p[4 * (size_t)st], p->d_g, dst(st),
                                p->gt.slots.dev, ng, b->n_rows, p->dims[(size_t)st], p->dims[(size_t)st + 1], s);
    if (rc != FDLP_OK) return rc;
  }
  if (mode != FDLP_NNET_RAW)
    HIP_TRY(fdlp::launch_row_epilogue((float*)b->out_dev, b->n_rows, p->dims[(size_t)p->n_stages], mode,
                                      (const float*)prior_dev, prior_weight, s));
  return FDLP_OK;
}

int fdlp_rnn_compute(fdlp_rnn_plan* p, const fdlp_post_batch* b, int32_t tap, int32_t mode, const void* prior_dev,
                     float prior_weight, void* stream) {
  if (!p || !b) return fail(FDLP_E_INVALID, "fdlp_rnn_compute: null argument");
  return stage_compute(p, b, tap, mode, prior_dev, prior_weight, stream);
}

// ---------------------------------------------------------------------------------------------
// Network plan (cmvn | deltas | splice | nnetFeedforward): the stage plan with the stages linear_relu x
// (n_linear - 1), linear.  fdlp_nnet_plan is that plan under the name include/fdlp.h gives this front.
// ---------------------------------------------------------------------------------------------
static fdlp_rnn_plan* stage_plan(fdlp_nnet_plan* p) { return reinterpret_cast<fdlp_rnn_plan*>(p); }

int fdlp_nnet_plan_create(const fdlp_nnet_config* cfg, const float* const* weights, const float* const* biases,
                          int64_t max_rows, fdlp_nnet_plan** out) {
  static_assert(FDLP_NNET_MAX_LINEAR <= FDLP_RNN_MAX_STAGES, "a layer is a stage");
  if (!cfg || !out) return fail(FDLP_E_INVALID, "fdlp_nnet_plan_create: null argument");
  *out = nullptr;
  const int nl = cfg->n_linear;
  if (nl < 1 || nl > FDLP_NNET_MAX_LINEAR)
    return fail(FDLP_E_INVALID, "the network needs 1 .. " + std::to_string(FDLP_NNET_MAX_LINEAR) +
                                    " linear layers, got n_linear = " + std::to_string(nl));
  fdlp_rnn_config sc{};
  sc.post = cfg->post;
  sc.n_stages = nl;
  for (int l = 0; l < nl; ++l) sc.kind[l] = l + 1 < nl ? FDLP_RNN_LINEAR_RELU : FDLP_RNN_LINEAR;
  std::copy(cfg->dims, cfg->dims + nl + 1, sc.dims);
  std::vector<const float*> params;
  if (weights && biases) {
    params.assign(4 * (size_t)nl, nullptr);
    for (int l = 0; l < nl; ++l) {
      params[4 * (size_t)l] = weights[l];
      params[4 * (size_t)l + 2] = biases[l];
    }
  }
  fdlp_rnn_plan* p = nullptr;
  const int rc = stage_plan_create(&sc, params.empty() ? nullptr : params.data(), max_rows, 0, kNnetWords, &p);
  *out = reinterpret_cast<fdlp_nnet_plan*>(p);
  return rc;
}

int fdlp_nnet_plan_destroy(fdlp_nnet_plan* p) { return fdlp_rnn_plan_destroy(stage_plan(p)); }

int fdlp_nnet_plan_info(const fdlp_nnet_plan* p, int32_t* in_dim, int32_t* n_linear, int32_t* out_dims,
                        int64_t* workspace_bytes, int32_t* tile, int32_t* lds_bytes) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_nnet_plan_info: null plan");
  stage_plan_sizes(stage_plan(const_cast<fdlp_nnet_plan*>(p)), in_dim, n_linear, out_dims, workspace_bytes);
  if (tile) {
    tile[0] = fdlp::kDenseTM;
    tile[1] = fdlp::kDenseTN;
    tile[2] = fdlp::kDenseKC;
  }
  if (lds_bytes) *lds_bytes = (int32_t)fdlp::dense_lds_bytes(fdlp::kDenseTN);
  return FDLP_OK;
}

int fdlp_nnet_compute(fdlp_nnet_plan* p, const fdlp_post_batch* b, int32_t tap, int32_t mode, const void* prior_dev,
                      float prior_weight, void* stream) {
  if (!p || !b) return fail(FDLP_E_INVALID, "fdlp_nnet_compute: null argument");
  return stage_compute(stage_plan(p), b, tap, mode, prior_dev, prior_weight, stream);
}

// ---------------------------------------------------------------------------------------------
// VAE-encoded plan (compute_vae_encoded_likelihood.py): the stage plan with the stages
//   encoder (GRU x n_enc_layers | conv x n_conv), means (linear), norm, GRU x n_cls_layers, regression (linear).
// fdlp_venc_plan is that plan under the name include/fdlp.h gives this front.
// ---------------------------------------------------------------------------------------------
static fdlp_rnn_plan* stage_plan(fdlp_venc_plan* p) { return reinterpret_cast<fdlp_rnn_plan*>(p); }
static const fdlp_rnn_plan* stage_plan(const fdlp_venc_plan* p) { return reinterpret_cast<const fdlp_rnn_plan*>(p); }

int fdlp_venc_create(const fdlp_venc_config* cfg, const float* const* params, int64_t max_rows, int32_t max_utts,
                          fdlp_venc_plan** out) {
  if (!cfg || !out) return fail(FDLP_E_INVALID, "fdlp_venc_create: null argument");
  *out = nullptr;
  if (max_utts < 1) return fail(FDLP_E_INVALID, "max_utts must be >= 1, got " + std::to_string(max_utts));
  const bool cnn = cfg->arch == FDLP_VENC_CNN;
  if (!cnn && cfg->arch != FDLP_VENC_RNN)
    return fail(FDLP_E_INVALID, "unknown encoder arch " + std::to_string(cfg->arch) + " (0 RNN, 1 CNN)");
  const int ne = cnn ? cfg->n_conv : cfg->n_enc_layers, nc = cfg->n_cls_layers;
  if (cnn && (ne < 1 || ne > FDLP_VENC_MAX_CONV))
    return fail(FDLP_E_INVALID, "the CNN encoder needs 1 .. " + std::to_string(FDLP_VENC_MAX_CONV) +
                                    " convolutions, got n_conv = " + std::to_string(ne));
  if (ne < 1 || nc < 1 || ne + nc + 3 > FDLP_RNN_MAX_STAGES)
    return fail(FDLP_E_INVALID, "the model needs at least one encoder and one classifier layer and at most " +
                                    std::to_string(FDLP_RNN_MAX_STAGES) + " stages, got " + std::to_string(ne) +
                                    " + means + norm + " + std::to_string(nc) + " + regression");
  fdlp_rnn_config sc{};
  sc.post = cfg->post;
  sc.n_stages = ne + nc + 3;
  ConvGeom cg{cfg->feat_h, cfg->kh, cfg->kw};
  int s = 0;
  if (cnn) {
    if (cfg->kh < 1 || cfg->kw < 1 || cfg->kh % 2 == 0 || cfg->kw % 2 == 0)
      return fail(FDLP_E_INVALID, "a same-padded convolution needs an odd kernel, got (" + std::to_string(cfg->kh) +
                                      ", " + std::to_string(cfg->kw) + ")");
    if (cfg->channels[0] != 1)
      return fail(FDLP_E_INVALID, "the first convolution reads the one-channel feature image, got channels[0] = " +
                                      std::to_string(cfg->channels[0]));
    if (cfg->feat_h < 1) return fail(FDLP_E_INVALID, "feat_h must be >= 1, got " + std::to_string(cfg->feat_h));
    for (int l = 0; l <= ne; ++l) {
      if (cfg->channels[l] < 1 || (int64_t)cfg->channels[l] * cfg->feat_h > INT32_MAX)
        return fail(FDLP_E_INVALID, "channels[" + std::to_string(l) + "] = " + std::to_string(cfg->channels[l]) +
                                        " at height " + std::to_string(cfg->feat_h) + " is outside 1 .. 2^31 - 1 columns");
      sc.dims[l] = cfg->channels[l] * cfg->feat_h;
    }
    for (; s < ne; ++s) sc.kind[s] = kStageConv;
  } else {
    sc.dims[0] = cfg->in_dim;
    for (; s < ne; ++s) {
      sc.kind[s] = FDLP_RNN_GRU;
      sc.dims[s + 1] = cfg->enc_hidden;
    }
  }
  sc.kind[s] = FDLP_RNN_LINEAR; sc.dims[++s] = cfg->latent_dim;   // means
  sc.kind[s] = kStageNorm; sc.dims[++s] = cfg->latent_dim;
  for (int l = 0; l < nc; ++l) {
    sc.kind[s] = FDLP_RNN_GRU;
    sc.dims[++s] = cfg->cls_hidden;
  }
  sc.kind[s] = FDLP_RNN_LINEAR; sc.dims[++s] = cfg->n_classes;    // regression
  fdlp_rnn_plan* p = nullptr;
  const int rc = stage_plan_create(&sc, params, max_rows, max_utts, kVencWords, &p, &cg);
  *out = reinterpret_cast<fdlp_venc_plan*>(p);
  return rc;
}

int fdlp_venc_plan_destroy(fdlp_venc_plan* p) { return fdlp_rnn_plan_destroy(stage_plan(p)); }

int fdlp_venc_plan_info(const fdlp_venc_plan* vp, int32_t* in_dim, int32_t* n_stages, int32_t* out_dims,
                        int64_t* workspace_bytes, int32_t* group_utts, int32_t* lds_bytes) {
  if (!vp) return fail(FDLP_E_INVALID, "fdlp_venc_plan_info: null plan");
  const fdlp_rnn_plan* p = stage_plan(vp);
  stage_plan_sizes(p, in_dim, n_stages, out_dims, workspace_bytes);
  if (group_utts) *group_utts = fdlp::kGruGU;
  if (lds_bytes) {
    lds_bytes[0] = p->max_h ? (int32_t)fdlp::gru_lds_bytes(p->max_h) : 0;
    lds_bytes[1] = (int32_t)p->conv_lds;
  }
  return FDLP_OK;
}

int fdlp_venc_plan_groups(const fdlp_venc_plan* p, const int32_t* lengths, int32_t n_utts, int32_t* group_of,
                          int32_t* slot_of, int32_t* n_groups) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_venc_plan_groups: bad arguments");
  return group_table_of("fdlp_venc_plan_groups", lengths, n_utts, group_of, slot_of, n_groups);
}

int fdlp_venc_compute(fdlp_venc_plan* p, const fdlp_post_batch* b, int32_t tap, int32_t mode, const void* prior_dev,
                      float prior_weight, void* stream) {
  if (!p || !b) return fail(FDLP_E_INVALID, "fdlp_venc_compute: null argument");
  return stage_compute(stage_plan(p), b, tap, mode, prior_dev, prior_weight, stream);
}

int fdlp_venc_set_profiling(fdlp_venc_plan* p, int32_t on) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_venc_set_profiling: null plan");
  stage_plan(p)->lm.profile = on != 0;
  return FDLP_OK;
}

int fdlp_venc_times(fdlp_venc_plan* p, double* ms) {
  if (!p || !ms) return fail(FDLP_E_INVALID, "fdlp_venc_times: null argument");
  DeviceGuard dg(stage_plan(p)->device);
  return stage_plan(p)->lm.times(ms, 3);
}

// ---------------------------------------------------------------------------------------------
// Multi-stream plan (nnetRNNMultimod): n_streams chains, each into its own sub-network of n_sub_layers GRUs of
// width Hs, whose outputs lie side by side in one [rows, M Hs] buffer that the trunk (n_trunk_layers GRUs of width
// M Hs and the regression) reads.  The sub-network scans of all streams are ONE launch per layer
// (launch_gru_scan_streams); the last one writes stream s at column s Hs of the concatenated buffer.  The trunk is
// the stage plan's own stage_launch; the group table, the marks and the checks are the stage plan's too.
//   d_g   [max_rows, 3 M Hs]: the sub-networks' M projection buffers [max_rows, 3 Hs] one after another, then the
//         trunk's one projection buffer
//   d_x   two [max_rows, M Hs]: X_0 the concatenation, X_t trunk GRU t's output, in d_x[t & 1] (the tapped one in
//         out_dev); a sub-network layer before the last writes M compact [max_rows, Hs] buffers into the one of the
//         two that the next layer does not write
// ---------------------------------------------------------------------------------------------
static const StageWords kMmodWords = {"fdlp_mmod_plan_create", "fdlp_mmod_compute", "model", "tap"};

struct fdlp_mmod_plan {
  int M = 0, Ls = 0, Hs = 0, Lt = 0, C = 0, K0 = 0, device = -1;
  int64_t max_rows = 0;
  int max_utts = 0;
  std::vector<std::unique_ptr<fdlp_xform_plan>> l0;  // per stream: its chain with layer 0's [W_ih | b_ih] as the transform
  std::vector<float*> d_m0;          // per stream [3 Hs, K0 + 1]
  std::vector<float*> d_sub;         // 4 per (stream, layer): w_ih, w_hh, b_ih, b_hh (layer 0: w_hh and b_hh only)
  std::vector<float*> d_trunk;       // 4 per trunk GRU, then the regression's {w, null, b, null}
  float* d_g = nullptr;
  float* d_x[2] = {nullptr, nullptr};
  GroupTable gt;
  LaunchMarks lm;
  DeviceResources res;
};

int fdlp_mmod_plan_create(const fdlp_mmod_config* cfg, const float* const* params, int64_t max_rows, int32_t max_utts,
                          fdlp_mmod_plan** out) {
  if (!cfg || !out) return fail(FDLP_E_INVALID, "fdlp_mmod_plan_create: null argument");
  *out = nullptr;
  const int M = cfg->n_streams, Ls = cfg->n_sub_layers, Hs = cfg->hidden_sub, Lt = cfg->n_trunk_layers;
  if (M < 1 || M > FDLP_MMOD_MAX_STREAMS)
    return fail(FDLP_E_INVALID, "the model needs 1 .. " + std::to_string(FDLP_MMOD_MAX_STREAMS) +
                                    " streams, got n_streams = " + std::to_string(M));
  if (Ls < 1 || Ls > FDLP_RNN_MAX_STAGES || Lt < 0 || Lt > FDLP_RNN_MAX_STAGES)
    return fail(FDLP_E_INVALID, "the model needs n_sub_layers in 1 .. " + std::to_string(FDLP_RNN_MAX_STAGES) +
                                    " and n_trunk_layers in 0 .. " + std::to_string(FDLP_RNN_MAX_STAGES) + ", got " +
                                    std::to_string(Ls) + " and " + std::to_string(Lt));
  if (Hs < 1 || cfg->n_classes < 1 || cfg->in_dim < 1)
    return fail(FDLP_E_INVALID, "hidden_sub " + std::to_string(Hs) + ", n_classes " + std::to_string(cfg->n_classes) +
                                    ", in_dim " + std::to_string(cfg->in_dim) + ": every dimension must be >= 1");
  const int64_t HT = (int64_t)M * Hs;
  if (Hs > fdlp::gru_max_hidden() || HT > fdlp::gru_max_hidden())
    return fail(FDLP_E_INVALID, std::to_string(M) + " streams of " + std::to_string(Hs) + " hidden units give a "
                                    "trunk GRU of " + std::to_string(HT) + "; the widest the 163840-byte LDS holds "
                                    "has " + std::to_string(fdlp::gru_max_hidden()));
  if (max_rows < 1) return fail(FDLP_E_INVALID, "max_rows must be >= 1, got " + std::to_string(max_rows));
  if (max_utts < 1) return fail(FDLP_E_INVALID, "max_utts must be >= 1, got " + std::to_string(max_utts));
  const int device = cfg->post[0].device;
  const bool dev = device >= 0;
  const size_t n_params = 4 * ((size_t)M * Ls + Lt) + 2;
  if (dev && !params) return fail(FDLP_E_INVALID, "fdlp_mmod_plan_create: null parameters");
  for (size_t i = 0; dev && i < n_params; ++i)
    if (!params[i]) return fail(FDLP_E_INVALID, "fdlp_mmod_plan_create: null parameter " + std::to_string(i));
  PlanPtr<fdlp_mmod_plan> p(new (std::nothrow) fdlp_mmod_plan);
  if (!p) return fail(FDLP_E_NOMEM, "out of memory");
  p->M = M; p->Ls = Ls; p->Hs = Hs; p->Lt = Lt; p->C = cfg->n_classes; p->K0 = cfg->in_dim; p->device = p->res.device = device;
  p->max_rows = max_rows;
  p->max_utts = max_utts;
  p->gt.max_groups = (max_utts + fdlp::kGruGU - 1) / fdlp::kGruGU;
  int rc;
  for (int s = 0; s < M; ++s) {
    fdlp_xform_config xc{};
    xc.post = cfg->post[s];
    xc.post.device = device;
    xc.out_dim = 3 * Hs;
    xc.affine = 1;
    fdlp_xform_plan* x = nullptr;
    if ((rc = fdlp_xform_plan_create(&xc, &x)) != FDLP_OK) {
      fdlp::last_error_slot() = "stream " + std::to_string(s) + ": " + fdlp::last_error_slot();
      return rc;
    }
    p->l0.emplace_back(x);
    if (x->post->Dout != p->K0)
      return fail(FDLP_E_INVALID, "stream " + std::to_string(s) + " gives " + std::to_string(x->post->Dout) +
                                      " spliced columns where the sub-networks take in_dim = " +
                                      std::to_string(p->K0));
  }
  if (!dev) {
    *out = p.release();
    return FDLP_OK;
  }
  DeviceGuard dg(device);
  if (dg.status() != hipSuccess) return fail(FDLP_E_HIP, "hipSetDevice failed");
  DeviceResources& res = p->res;
  const int K0 = p->K0;
  p->d_m0.assign((size_t)M, nullptr);
  p->d_sub.assign(4 * (size_t)M * Ls, nullptr);
  p->d_trunk.assign(4 * ((size_t)Lt + 1), nullptr);
  for (int s = 0; s < M; ++s) {
    for (int l = 0; l < Ls; ++l) {
      const float* const* w = params + 4 * ((size_t)s * Ls + l);
      float** d = &p->d_sub[4 * ((size_t)s * Ls + l)];
      const size_t K = l == 0 ? (size_t)K0 : (size_t)Hs, H = (size_t)Hs;
      if (l == 0) {
        std::vector<float> m0(3 * H * (K + 1));  // [W_ih | b_ih], transform-feats' affine matrix
        for (size_t n = 0; n < 3 * H; ++n) {
          memcpy(&m0[n * (K + 1)], w[0] + n * K, sizeof(float) * K);
          m0[n * (K + 1) + K] = w[2][n];
        }
        if ((rc = upload(res, &p->d_m0[(size_t)s], m0.data(), m0.size())) != FDLP_OK) return rc;
      } else {
        if ((rc = upload(res, &d[0], w[0], 3 * H * K)) != FDLP_OK || (rc = upload(res, &d[2], w[2], 3 * H)) != FDLP_OK) return rc;
      }
      if ((rc = upload(res, &d[1], w[1], 3 * H * H)) != FDLP_OK || (rc = upload(res, &d[3], w[3], 3 * H)) != FDLP_OK) return rc;
    }
  }
  const size_t H = (size_t)HT;
  for (int l = 0; l < Lt; ++l) {
    const float* const* w = params + 4 * ((size_t)M * Ls + l);
    float** d = &p->d_trunk[4 * (size_t)l];
    const size_t count[4] = {3 * H * H, 3 * H * H, 3 * H, 3 * H};
    for (int i : {0, 2, 1, 3})
      if ((rc = upload(res, &d[i], w[i], count[i])) != FDLP_OK) return rc;
  }
  {
    const float* const* w = params + 4 * ((size_t)M * Ls + Lt);
    float** d = &p->d_trunk[4 * (size_t)Lt];
    if ((rc = upload(res, &d[0], w[0], (size_t)p->C * H)) != FDLP_OK || (rc = upload(res, &d[2], w[1], (size_t)p->C)) != FDLP_OK)
      return rc;
  }
  if ((rc = zeroed_workspace(res, &p->d_g, (size_t)max_rows * 3 * H, "the projection buffers", max_rows)) != FDLP_OK)
    return rc;
  for (float*& x : p->d_x)
    if ((rc = zeroed_workspace(res, &x, (size_t)max_rows * H, "a stage workspace", max_rows)) != FDLP_OK) return rc;
  if ((rc = p->gt.alloc(res)) != FDLP_OK) return rc;
  *out = p.release();
  return FDLP_OK;
}

int fdlp_mmod_plan_destroy(fdlp_mmod_plan* p) { delete p; return FDLP_OK; }

int fdlp_mmod_plan_info(const fdlp_mmod_plan* p, int32_t* in_dim, int32_t* n_taps, int32_t* tap_dims,
                        int64_t* workspace_bytes, int32_t* group_utts, int32_t* lds_bytes) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_mmod_plan_info: null plan");
  const int HT = p->M * p->Hs;
  if (in_dim) *in_dim = p->K0;
  if (n_taps) *n_taps = p->Lt + 2;
  if (tap_dims)
    for (int t = 0; t < p->Lt + 2; ++t) tap_dims[t] = t == 0 ? p->C : HT;
  if (workspace_bytes) *workspace_bytes = (int64_t)sizeof(float) * p->max_rows * 5 * HT + p->gt.bytes();
  if (group_utts) *group_utts = fdlp::kGruGU;
  if (lds_bytes) *lds_bytes = (int32_t)fdlp::gru_lds_bytes(p->Lt > 0 ? HT : p->Hs);
  return FDLP_OK;
}

int fdlp_mmod_plan_groups(const fdlp_mmod_plan* p, const int32_t* lengths, int32_t n_utts, int32_t* group_of,
                          int32_t* slot_of, int32_t* n_groups) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_mmod_plan_groups: bad arguments");
  return group_table_of("fdlp_mmod_plan_groups", lengths, n_utts, group_of, slot_of, n_groups);
}

int fdlp_mmod_set_profiling(fdlp_mmod_plan* p, int32_t on) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_mmod_set_profiling: null plan");
  p->lm.profile = on != 0;
  return FDLP_OK;
}

int fdlp_mmod_times(fdlp_mmod_plan* p, double* ms) {
  if (!p || !ms) return fail(FDLP_E_INVALID, "fdlp_mmod_times: null argument");
  DeviceGuard dg(p->device);
  return p->lm.times(ms);
}

int fdlp_mmod_compute(fdlp_mmod_plan* p, const fdlp_post_batch* bs, int32_t tap, int32_t mode, const void* prior_dev,
                      float prior_weight, void* stream) {
  if (!p || !bs) return fail(FDLP_E_INVALID, "fdlp_mmod_compute: null argument");
  if (p->device < 0) return fail(FDLP_E_INVALID, "fdlp_mmod_compute: host-only plan");
  const fdlp_post_batch* b = &bs[0];  // the batch whose table the scans use, and whose out_dev is the output
  {
    const int rc = stage_check_call(kMmodWords, p->Lt + 2, tap, mode, prior_dev, b, p->max_utts, p->max_rows, true);
    if (rc != FDLP_OK) return rc;
  }
  for (int s = 1; s < p->M; ++s) {
    const fdlp_post_batch& o = bs[s];
    if (o.n_utt != b->n_utt || o.n_rows != b->n_rows)
      return fail(FDLP_E_INVALID, "stream " + std::to_string(s) + " holds " + std::to_string(o.n_utt) +
                                      " utterances in " + std::to_string(o.n_rows) + " rows where stream 0 holds " +
                                      std::to_string(b->n_utt) + " in " + std::to_string(b->n_rows));
    if (o.n_utt > 0 && (!o.row_off || !o.utt_len)) return fail(FDLP_E_INVALID, "fdlp_mmod_compute: bad batch");
    for (int u = 0; u < o.n_utt; ++u)
      if (o.utt_len[u] != b->utt_len[u] || o.row_off[u] != b->row_off[u])
        return fail(FDLP_E_INVALID, "utterance " + std::to_string(u) + " has " + std::to_string(o.utt_len[u]) +
                                        " rows at row " + std::to_string(o.row_off[u]) + " in stream " +
                                        std::to_string(s) + " and " + std::to_string(b->utt_len[u]) + " at row " +
                                        std::to_string(b->row_off[u]) + " in stream 0");
  }
  const int M = p->M, Hs = p->Hs, HT = M * Hs, Ls = p->Ls;
  const int last = p->Lt + 1 - tap;  // the tapped X_t: 0 the concatenation, 1 .. Lt the trunk GRUs, Lt + 1 the logits
  hipStream_t s = (hipStream_t)stream;
  auto dst = [&](int t) { return t == last ? (float*)b->out_dev : p->d_x[t & 1]; };
  DeviceGuard dg(p->device);
  HIP_TRY(dg.status());
  LaunchMarks& lm = p->lm;
  const size_t gs = (size_t)p->max_rows * 3 * Hs, cs = (size_t)p->max_rows * Hs;  // a stream's share of d_g, d_x[i]
  // every stream's cmvn | splice | layer-0 projection in the chain's launch; its batch checks are the chain's
  fdlp::XformConsts xc{};
  xc.N = 3 * Hs; xc.C = p->K0 + 1; xc.affine = 1; xc.n_mat = 1;
  for (int st = 0; st < M; ++st) {
    fdlp_post_batch b0 = bs[st];
    b0.out_dev = p->d_g + st * gs;
    HIP_TRY(lm.begin(s));
    const int rc = post_compute(p->l0[(size_t)st]->post.get(), &b0, stream, &xc, p->d_m0[(size_t)st], nullptr);
    if (rc != FDLP_OK) return rc;
    HIP_TRY(lm.end(0, s));
  }
  if (b->n_utt == 0 || b->n_rows == 0) return FDLP_OK;
  int ng = 0;
  {
    const int rc = p->gt.stage(b, s, &ng);
    if (rc != FDLP_OK) return rc;
  }
  for (int l = 0; l < Ls; ++l) {
    // layers before the last: compact buffers, in the d_x the next layer does not write
    float* compact = p->d_x[(Ls - 1 - l) & 1];
    const float* in = p->d_x[(Ls - l) & 1];
    const bool cat = l == Ls - 1;
    fdlp::GruStreams gst{};
    for (int st = 0; st < M; ++st) {
      float* const* w = &p->d_sub[4 * ((size_t)st * Ls + l)];
      if (l > 0) {
        HIP_TRY(lm.begin(s));
        HIP_TRY(fdlp::launch_dense(in + st * cs, w[0], w[2], p->d_g + st * gs, b->n_rows, Hs, 3 * Hs, 0, s));
        HIP_TRY(lm.end(0, s));
      }
      gst.s[st] = {p->d_g + st * gs, w[1], w[3], cat ? dst(0) + (size_t)st * Hs : compact + st * cs};
    }
    HIP_TRY(lm.begin(s));
    HIP_TRY(fdlp::launch_gru_scan_streams(gst, M, cat ? HT : Hs, p->gt.slots.dev, ng, b->n_rows, Hs, s));
    HIP_TRY(lm.end(1, s));
  }
  for (int t = 1; t <= last; ++t) {
    const bool gru = t <= p->Lt;
    const int rc = stage_launch(lm, gru, p->d_x[(t - 1) & 1], 0, &p->d_trunk[4 * (size_t)(t - 1)], p->d_g, dst(t),
                                p->gt.slots.dev, ng, b->n_rows, HT, gru ? HT : p->C, s);
    if (rc != FDLP_OK) return rc;
  }
  if (mode != FDLP_NNET_RAW)
    HIP_TRY(fdlp::launch_row_epilogue((float*)b->out_dev, b->n_rows, p->C, mode, (const float*)prior_dev,
                                      prior_weight, s));
  return FDLP_OK;
}

// ---------------------------------------------------------------------------------------------
// The multi-domain tools (fdlp_lifelong.hip): stateless fronts of the four kernels; the work runs on the
// device that is current, as the pointers belong to it
// ---------------------------------------------------------------------------------------------
int fdlp_life_mmeasure(const float* post, int32_t n_models, int64_t n_rows, int32_t n_classes, int32_t n_utt,
                       const int64_t* row_off, const int64_t* utt_len, double* out, void* stream) {
  if (n_utt < 0 || n_rows < 0) return fail(FDLP_E_INVALID, "fdlp_life_mmeasure: negative n_utt or n_rows");
  if (n_utt == 0) return FDLP_OK;
  if (n_models < 1 || n_models > FDLP_LIFE_MAX_MODELS || n_classes < 1 || n_utt > 65535 || !post || !row_off ||
      !utt_len || !out)
    return fail(FDLP_E_INVALID, "fdlp_life_mmeasure: need 1 .. " + std::to_string(FDLP_LIFE_MAX_MODELS) +
                                    " models, n_classes >= 1, at most 65535 utterances and no null pointer (got " +
                                    std::to_string(n_models) + " models, " + std::to_string(n_classes) + " classes, " +
                                    std::to_string(n_utt) + " utterances)");
  hipStream_t s = (hipStream_t)stream;
  double* part = nullptr;  // stream-ordered scratch for the tile partials
  const size_t n = (size_t)8 * (size_t)n_utt * (size_t)n_models * (size_t)fdlp::mmeasure_tiles(n_classes);
  HIP_TRY(hipMallocAsync((void**)&part, sizeof(double) * n, s));
  hipError_t e = fdlp::launch_mmeasure(post, n_models, n_rows, n_classes, n_utt, row_off, utt_len, part, out, s);
  hipError_t e2 = hipFreeAsync(part, s);
  if (e != hipSuccess) return fail(FDLP_E_HIP, std::string("mmeasure kernels: ") + hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(FDLP_E_HIP, std::string("hipFreeAsync: ") + hipGetErrorString(e2));
  return FDLP_OK;
}

int fdlp_life_vae_sample(const float* ml, const float* eps, float* z, int64_t n_rows, int32_t bn, void* stream) {
  if (n_rows < 0 || bn < 1 || (n_rows > 0 && (!ml || !eps || !z)))
    return fail(FDLP_E_INVALID, "fdlp_life_vae_sample: need n_rows >= 0, bn >= 1 and no null pointer");
  HIP_TRY(fdlp::launch_vae_sample(ml, eps, z, n_rows, bn, (hipStream_t)stream));
  return FDLP_OK;
}

int fdlp_life_vae_elbo(const float* x, const float* xhat, const float* ml, int64_t n_rows, int32_t in_dim, int32_t bn,
                       int32_t n_utt, const int64_t* row_off, const int64_t* utt_len, int32_t mode, float* elbo,
                       double* out, int32_t ld_out, void* stream) {
  if (n_rows < 0 || n_utt < 0 || in_dim < 1 || bn < 1 || ld_out < 1 || (mode != FDLP_LIFE_LIFELONG && mode != FDLP_LIFE_INCREMENTAL))
    return fail(FDLP_E_INVALID, "fdlp_life_vae_elbo: need n_rows, n_utt >= 0, in_dim, bn, ld_out >= 1 and a known mode");
  if ((n_rows > 0 && (!x || !xhat || !ml || !elbo)) || (n_utt > 0 && (!row_off || !utt_len || !out || !elbo)))
    return fail(FDLP_E_INVALID, "fdlp_life_vae_elbo: null pointer");
  HIP_TRY(fdlp::launch_vae_elbo(x, xhat, ml, elbo, n_rows, in_dim, bn, n_utt, row_off, utt_len, mode, out, ld_out,
                                (hipStream_t)stream));
  return FDLP_OK;
}

int fdlp_life_fuse(const float* post, int32_t n_models, int64_t n_rows, int32_t n_classes, int32_t n_utt,
                   int64_t max_len, const int64_t* row_off, const int64_t* utt_len, const double* w, const double* tab,
                   double prior_weight, int32_t mode, float* out, void* stream) {
  if (n_utt < 0 || n_rows < 0 || max_len < 0) return fail(FDLP_E_INVALID, "fdlp_life_fuse: negative n_utt, n_rows or max_len");
  if (n_utt == 0 || max_len == 0) return FDLP_OK;
  if (n_models < 1 || n_models > FDLP_LIFE_MAX_MODELS || n_classes < 1 || !post || !row_off || !utt_len || !w || !tab ||
      !out || (mode != FDLP_LIFE_LIFELONG && mode != FDLP_LIFE_INCREMENTAL))
    return fail(FDLP_E_INVALID, "fdlp_life_fuse: need 1 .. " + std::to_string(FDLP_LIFE_MAX_MODELS) +
                                    " models, n_classes >= 1, a known mode and no null pointer (got " +
                                    std::to_string(n_models) + " models, " + std::to_string(n_classes) + " classes)");
  HIP_TRY(fdlp::launch_lifelong_fuse(post, n_models, n_rows, n_classes, n_utt, max_len, row_off, utt_len, w, tab,
                                     prior_weight, mode, out, (hipStream_t)stream));
  return FDLP_OK;
}
