// fdlp_plan_common.h -- what the plan translation units (fdlp_plan*.cpp, fdlp_tables.cpp) share: the HIP error
// idiom, device scoping, the owner of a plan's device resources with the one teardown protocol, the pinned
// staging table, frame geometry, and the declarations that cross the files.  Host C++, private to csrc/.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <optional>
#include <string>
#include <vector>

#include "../../include/fdlp.h"
#include "fdlp_error.h"
#include "fdlp_internal.h"

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return fdlp::fail(FDLP_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
  } while (0)

namespace fdlp {
namespace host {

// Makes `dev` current for the scope of an ABI call and restores the caller's device afterwards.
class DeviceGuard {
 public:
  explicit DeviceGuard(int dev) {
    if (dev < 0) return;
    if ((err_ = hipGetDevice(&prev_)) != hipSuccess) return;
    if (prev_ != dev) {
      err_ = hipSetDevice(dev);
      switched_ = err_ == hipSuccess;
    }
  }
  ~DeviceGuard() {
    if (switched_) (void)hipSetDevice(prev_);
  }
  hipError_t status() const { return err_; }

 private:
  int prev_ = -1;
  bool switched_ = false;
  hipError_t err_ = hipSuccess;
};

// A plan's first use of its device: the device exists and is current (in `dg`) until create returns
inline int open_device(int device, std::optional<DeviceGuard>& dg) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(FDLP_E_HIP, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(FDLP_E_INVALID, "device index out of range");
  dg.emplace(device);
  if (dg->status() != hipSuccess) return fail(FDLP_E_HIP, "hipSetDevice failed");
  return FDLP_OK;
}

// Owner of everything a plan holds on its device: each buffer, event and stream it hands out is recorded and
// released by the destructor, whether the plan was finished, half-built, or grew buffers after creation.  Every
// plan holds one by value and keeps typed raw pointers for its kernels' argument structs.  Teardown is one
// protocol: the plan's device current, hipDeviceSynchronize(), release, the caller's device back.  A plan that
// was handed nothing (host-only plans, device < 0) makes no HIP call.
class DeviceResources {
 public:
  int device = -1;  // the owning plan's

  DeviceResources() = default;
  DeviceResources(const DeviceResources&) = delete;
  DeviceResources& operator=(const DeviceResources&) = delete;
  ~DeviceResources() { release(); }

  template <typename T>
  hipError_t device_array(T** p, size_t n) {
    const hipError_t e = hipMalloc((void**)p, sizeof(T) * n);
    if (e == hipSuccess) dev_.push_back(*p);
    return e;
  }
  template <typename T>
  hipError_t pinned_array(T** p, size_t n) {
    const hipError_t e = hipHostMalloc((void**)p, sizeof(T) * n, hipHostMallocDefault);
    if (e == hipSuccess) pin_.push_back(*p);
    return e;
  }
  hipError_t event(hipEvent_t* ev) {  // ordering only, no timing
    const hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e == hipSuccess) ev_.push_back(*ev);
    return e;
  }
  hipError_t stream(hipStream_t* s) {
    const hipError_t e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    if (e == hipSuccess) st_.push_back(*s);
    return e;
  }
  // gives back one array early (a table that is outgrown); the caller has made sure nothing reads it
  void drop_device_array(void* p) {
    auto it = std::find(dev_.begin(), dev_.end(), p);
    if (it == dev_.end()) return;
    dev_.erase(it);
    (void)hipFree(p);
  }
  void drop_pinned_array(void* p) {
    auto it = std::find(pin_.begin(), pin_.end(), p);
    if (it == pin_.end()) return;
    pin_.erase(it);
    (void)hipHostFree(p);
  }
  void release() {
    if (dev_.empty() && pin_.empty() && ev_.empty() && st_.empty()) return;
    DeviceGuard dg(device);
    (void)hipDeviceSynchronize();
    for (void* p : dev_) (void)hipFree(p);
    for (void* p : pin_) (void)hipHostFree(p);
    for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
    for (hipStream_t s : st_) (void)hipStreamDestroy(s);
    dev_.clear(); pin_.clear(); ev_.clear(); st_.clear();
  }

 private:
  std::vector<void*> dev_, pin_;
  std::vector<hipEvent_t> ev_;
  std::vector<hipStream_t> st_;
};

template <typename T>
int upload(DeviceResources& res, T** dst, const T* src, size_t n) {
  HIP_TRY(res.device_array(dst, std::max<size_t>(n, 1)));
  if (n) HIP_TRY(hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice));
  return FDLP_OK;
}

// What a create function holds its plan in: an early return deletes the half-built plan (its destructor and its
// DeviceResources clean up), and the message of the error that ended it survives that.
struct PlanDeleter {
  template <typename P>
  void operator()(P* p) const {
    const std::string m = last_error_slot();
    delete p;
    last_error_slot() = m;
  }
};
template <typename P>
using PlanPtr = std::unique_ptr<P, PlanDeleter>;

// A table a compute call fills on the host and the batch's kernels read on the device: the pinned array, the
// device array, and the event after the copy, which the next call waits for before it overwrites `host`.
// A table without an event of its own (event() never called) is copied in front of one that has it.
template <typename T>
struct Staging {
  T* host = nullptr;
  T* dev = nullptr;
  size_t cap = 0;
  hipEvent_t done = nullptr;
  bool pending = false;

  hipError_t arrays(DeviceResources& res, size_t n) {
    hipError_t e = res.device_array(&dev, n);
    if (e == hipSuccess) e = res.pinned_array(&host, n);
    if (e == hipSuccess) cap = n;
    return e;
  }
  hipError_t event(DeviceResources& res) { return res.event(&done); }
  // room for n entries in a table that grows with its batches: max(n + n / 2, 1024)
  int reserve(DeviceResources& res, size_t n, const char* nomem_message) {
    if (n <= cap) return FDLP_OK;
    HIP_TRY(hipDeviceSynchronize());  // the previous batch's kernel may still read dev
    res.drop_device_array(dev);
    res.drop_pinned_array(host);
    dev = nullptr; host = nullptr; cap = 0;
    if (arrays(res, std::max<size_t>(n + n / 2, 1024)) != hipSuccess) return fail(FDLP_E_NOMEM, nomem_message);
    return FDLP_OK;
  }
  int wait() {  // host may still feed the previous call's copy
    if (pending) {
      HIP_TRY(hipEventSynchronize(done));
      pending = false;
    }
    return FDLP_OK;
  }
  int publish(size_t n, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(dev, host, sizeof(T) * n, hipMemcpyHostToDevice, s));
    if (done) {
      HIP_TRY(hipEventRecord(done, s));
      pending = true;
    }
    return FDLP_OK;
  }
};

// getFrames (features.py:134-151): frame length, hop and the reflected extension of the signal
struct FrameGrid {
  int L = 0, hop = 0, sp_b = 0, sp_f = 0, ext = 0;

  FrameGrid() = default;
  FrameGrid(int srate, double fduration, int hop_) : L((int)((double)srate * fduration)), hop(hop_) {  // :134
    if (L % 2 == 0) { sp_b = L / 2 - 1; sp_f = L / 2; ext = L / 2 - 1; }
    else { sp_b = sp_f = ext = (L - 1) / 2; }
  }
  // idx = sp_b + k*hop, yield while idx + sp_f < T + 2*ext  (:151)
  int64_t frames_of(int64_t T) const {
    const int64_t lim = T + 2 * (int64_t)ext - sp_b - sp_f;  // k*hop < lim
    if (lim <= 0) return 0;
    return (lim - 1) / hop + 1;
  }
};

// [lo, hi): the span of a filterbank row's taps with |tap| >= thr (thr = 0: the non-zero taps); 0, 0 without one
inline void band_support(const double* row, int width, double thr, int* lo, int* hi) {
  int a = width, b = 0;
  for (int m = 0; m < width; ++m) {
    const bool keep = thr > 0 ? std::fabs(row[m]) >= thr : row[m] != 0.0;
    if (keep) { a = std::min(a, m); b = m + 1; }
  }
  if (b <= a) { a = 0; b = 0; }
  *lo = a;
  *hi = b;
}

// The F frame descriptors (MelFrame, MfccFrame) of utterance u of batch b, T samples long; extra(frame) sets what
// only one of them has
template <typename Frame, typename Extra>
void fill_frames(Frame* dst, const fdlp_batch* b, int u, int64_t T, int64_t F, Extra extra) {
  for (int64_t k = 0; k < F; ++k) {
    Frame& fd = dst[k];
    fd.pcm_off = b->pcm_off[u];
    fd.noise_off = b->noise_dev ? b->noise_off[u] : -1;
    fd.alpha = b->noise_dev ? b->noise_alpha[u] : 0.0;
    fd.out_row = b->out_row[u] + k;
    fd.T = (int32_t)T;
    fd.k = (int32_t)k;
    extra(fd);
  }
}

// ---- fdlp_tables.cpp: the host table builders ----
std::vector<double> linspace(double start, double stop, int num);
std::vector<double> cos_window(int M, double c0, double c1);
std::vector<double> fbank_cochlear(int nf, int nfft, int srate, double om_w, double alp, int fixed, double bet,
                                   double wf, int* ncol_out);
std::vector<double> fbank_mel(int nf, int nfft, int srate, double wf, int* ncol_out);

// Structured-autocorrelation tables (DESIGN.md "Structured autocorrelation") for
// createFbankCochlear with fixed == 1: every band's taps must follow the lower-skirt / flat-top /
// upper-skirt pattern along m (classified exactly like fbank_cochlear), and the skirt factors
// E, E', K, K' must stay well inside the fp64 range.  skirt_tables returns false otherwise (direct path).
struct SkirtTables {
  std::vector<double> e;    // [2, N]
  std::vector<SkSnap> snap;  // [2, B] in sweep order
  std::vector<int2> reg;    // [B]
  int smin[2] = {0, 0};
  // flat-top sweep of ac_vsweep_kernel: events and chain count (C = 0: not possible)
  std::vector<FlatEv> fl;
  int fl_C = 0, fl_lo = 0, fl_hi = 0;
  int fl_H = 1;
  int part_lo[kMaxFlatParts] = {0}, part_hi[kMaxFlatParts] = {0}, part_ev[kMaxFlatParts + 1] = {0};
  std::vector<int2> fl_band;  // [B] (chain, partial-part mask)
  // wrap straddle: band j whose last nlags-1 taps lie on its upper skirt and first nlags-1 on its lower
  // skirt has straddle_N,j[l] = sqrt(K_j K'_j) Wrap[l], Wrap[l] = sum_{i<l} z[N-l+i] y[i] (one per frame);
  // wrap_kw[j] = sqrt(K_j K'_j) for those bands, 0 for the others (ac_band_kernel computes theirs)
  std::vector<double> wrap_kw;
  bool wrap_any = false;
};
bool skirt_tables(const fdlp_config& c, int B, int N, int nfft, SkirtTables* T);
bool factor_radices(int n, DftPlan* d);
bool split_four_step(int N, DftPlan* d1, DftPlan* d2);
double gamma_pdf(double x, double a, double loc, double scale);
void post_scale_tables(int order, int window, std::vector<int32_t>& lens, std::vector<float>& flat);
int ola_table(int kk, int kkb2, int ola_hop, int F, int L, const uint8_t* jit, int32_t* dst, int32_t* src,
              int32_t* cnt);

}  // namespace host
}  // namespace fdlp

// ---- fdlp_plan_post.cpp: the chain plans the model plans are built on ----
struct fdlp_post_plan {
  fdlp_post_config cfg{};
  int D = 0, Dp = 0, Dout = 0, tf = 0;
  size_t lds = 0;
  std::vector<int32_t> lens;
  std::vector<float> scales;  // concatenated tables
  fdlp::PostConsts pc{};
  float* d_scales = nullptr;
  fdlp::host::Staging<fdlp::PostTile> tiles;  // grows with the batches
  fdlp::host::DeviceResources res;
};

struct fdlp_xform_plan {
  std::unique_ptr<fdlp_post_plan> post;
  int N = 0, C = 0, affine = 0;
  size_t lds = 0;
};

namespace fdlp {
namespace host {
// xc: null for the plain chain; otherwise the transform's constants, with mats [xc->n_mat, N, C] on the device and
// mat_index[u] (host, or null for matrix 0) carried to the tiles like norm_index
int post_compute(fdlp_post_plan* p, const fdlp_post_batch* b, void* stream, const XformConsts* xc, const void* mats,
                 const int32_t* mat_index);
}  // namespace host
}  // namespace fdlp
