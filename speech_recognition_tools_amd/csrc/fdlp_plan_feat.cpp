// fdlp_plan_feat.cpp -- the sibling featurizers' plans: mel spectrum (computeMelSpectrum.py) and MFCC
// (computeMfccFeatures.py), one kernel each over a staged table of frame descriptors.
#include <string.h>

#include "fdlp_plan_common.h"

using fdlp::fail;
using namespace fdlp::host;

// ---------------------------------------------------------------------------------------------
// mel spectrum plan (computeMelSpectrum.py:40-170)
// ---------------------------------------------------------------------------------------------
struct fdlp_mel_plan {
  fdlp_mel_config cfg{};
  int device = 0;
  FrameGrid grid;
  int nbins = 0;
  fdlp::MelConsts mc{};
  double *d_win = nullptr, *d_fb = nullptr;
  int *d_lo = nullptr, *d_hi = nullptr;
  double2 *d_om = nullptr, *d_rtw = nullptr;
  Staging<fdlp::MelFrame> frames;
  DeviceResources res;
};

int fdlp_mel_plan_create(const fdlp_mel_config* cfg, int device, fdlp_mel_plan** out) {
  if (!cfg || !out) return fail(FDLP_E_INVALID, "fdlp_mel_plan_create: null argument");
  *out = nullptr;
  const fdlp_mel_config& c = *cfg;
  if (c.nfilters < 1 || c.srate < 1 || c.frate < 1 || !(c.fduration > 0) || c.max_frames < 1)
    return fail(FDLP_E_INVALID, "invalid mel configuration");
  if (c.nfft < 2 || c.nfft % 2 || c.nfft / 2 > 2048) return fail(FDLP_E_INVALID, "nfft must be even and <= 4096");
  PlanPtr<fdlp_mel_plan> p(new (std::nothrow) fdlp_mel_plan);
  if (!p) return fail(FDLP_E_NOMEM, "out of memory");
  p->cfg = c;
  p->device = p->res.device = device;
  p->grid = FrameGrid(c.srate, c.fduration, (int)((double)c.srate / (double)c.frate));  // features.py:135
  if (p->grid.L < 2 || p->grid.hop < 1) return fail(FDLP_E_INVALID, "frame length / hop too small");
  const int nh = c.nfft / 2;
  fdlp::DftPlan dp{};
  if (!factor_radices(nh, &dp)) return fail(FDLP_E_INVALID, "nfft/2 must factor into 2, 3, 5 and 7");
  std::vector<double> fb;
  int ncol = 0;
  if (c.fbank_kind == FDLP_FBANK_MEL) fb = fbank_mel(c.nfilters, c.nfft, c.srate, c.warp_fact, &ncol);  // :57
  else if (c.fbank_kind == FDLP_FBANK_COCHLEAR)
    fb = fbank_cochlear(c.nfilters, c.nfft, c.srate, c.om_w, c.alp, c.fixed, c.bet, c.warp_fact, &ncol);  // :63-65
  else return fail(FDLP_E_INVALID, "Invalid type of filter bank, use mel or cochlear with proper configuration");
  if (ncol != nh + 1) return fail(FDLP_E_INVALID, "filterbank width does not match nfft/2+1");
  p->nbins = ncol;
  std::vector<int> lo(c.nfilters, 0), hi(c.nfilters, 0);
  for (int m = 0; m < c.nfilters; ++m) band_support(&fb[(size_t)m * ncol], ncol, 0.0, &lo[m], &hi[m]);
  const std::vector<double> win = cos_window(p->grid.L, 0.54, 0.46);  // np.hamming (computeMelSpectrum.py:41)
  const long double PI = 3.141592653589793238462643383279502884L;
  std::vector<double2> om(nh), rtw(nh + 1);
  for (int q = 0; q < nh; ++q) {
    const long double ang = -2.0L * PI * (long double)q / (long double)nh;
    om[q] = make_double2((double)cosl(ang), (double)sinl(ang));
  }
  for (int k = 0; k <= nh; ++k) {
    const long double ang = -2.0L * PI * (long double)k / (long double)c.nfft;
    rtw[k] = make_double2((double)cosl(ang), (double)sinl(ang));
  }
  if (device < 0) {
    *out = p.release();
    return FDLP_OK;
  }
  std::optional<DeviceGuard> dg;
  int rc;
  if ((rc = open_device(device, dg)) != FDLP_OK) return rc;
  DeviceResources& res = p->res;
  if ((rc = upload(res, &p->d_win, win.data(), win.size())) != FDLP_OK) return rc;
  if ((rc = upload(res, &p->d_fb, fb.data(), fb.size())) != FDLP_OK) return rc;
  if ((rc = upload(res, &p->d_lo, lo.data(), lo.size())) != FDLP_OK) return rc;
  if ((rc = upload(res, &p->d_hi, hi.data(), hi.size())) != FDLP_OK) return rc;
  if ((rc = upload(res, &p->d_om, om.data(), om.size())) != FDLP_OK) return rc;
  if ((rc = upload(res, &p->d_rtw, rtw.data(), rtw.size())) != FDLP_OK) return rc;
  if (p->frames.arrays(res, (size_t)c.max_frames) != hipSuccess || p->frames.event(res) != hipSuccess)
    return fail(FDLP_E_NOMEM, "mel plan workspace allocation failed");
  fdlp::MelConsts& m = p->mc;
  m.L = p->grid.L; m.hop = p->grid.hop; m.ext = p->grid.ext; m.nfft = c.nfft; m.nh = nh; m.nbins = ncol;
  m.nfilters = c.nfilters; m.power = c.power ? 1 : 0;
  m.window = p->d_win; m.fbank = p->d_fb; m.lo = p->d_lo; m.hi = p->d_hi; m.om = p->d_om; m.rtw = p->d_rtw;
  m.dp = dp;
  *out = p.release();
  return FDLP_OK;
}

int fdlp_mel_plan_destroy(fdlp_mel_plan* p) { delete p; return FDLP_OK; }

int fdlp_mel_geometry(const fdlp_mel_plan* p, int64_t T, int32_t* F) {
  if (!p || !F || T < 0) return fail(FDLP_E_INVALID, "fdlp_mel_geometry: bad args");
  *F = (int32_t)p->grid.frames_of(T);
  return FDLP_OK;
}

int fdlp_mel_compute(fdlp_mel_plan* p, const fdlp_batch* b, void* stream) {
  if (!p || !b || p->device < 0) return fail(FDLP_E_INVALID, "fdlp_mel_compute: bad args or host-only plan");
  if (b->n_utt < 0 || (b->n_utt > 0 && (!b->pcm_dev || !b->pcm_off || !b->utt_len || !b->out_row)) ||
      (!b->out_dev && !b->out_f64_dev))
    return fail(FDLP_E_INVALID, "fdlp_mel_compute: bad batch");
  if (b->noise_dev && (!b->noise_off || !b->noise_alpha)) return fail(FDLP_E_INVALID, "noise arrays missing");
  if (b->preprocess == FDLP_PRE_DIFF && (b->pcm_kind != FDLP_PCM_I16 || b->noise_dev))
    return fail(FDLP_E_INVALID, "diff preprocessing needs int16 PCM and no noise");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard dg(p->device);  // the caller's current device is restored on return
  HIP_TRY(dg.status());
  int rc;
  if ((rc = p->frames.wait()) != FDLP_OK) return rc;
  int nf = 0;
  for (int u = 0; u < b->n_utt; ++u) {
    const int64_t T = b->utt_len[u];
    if (T < 1) return fail(FDLP_E_INVALID, "empty utterance");
    const int64_t F = p->grid.frames_of(T);
    if (nf + F > p->cfg.max_frames) return fail(FDLP_E_CAPACITY, "batch exceeds the mel plan's max_frames");
    fill_frames(p->frames.host + nf, b, u, T, F, [](fdlp::MelFrame&) {});
    nf += (int)F;
  }
  if (nf == 0) return FDLP_OK;
  if ((rc = p->frames.publish((size_t)nf, s)) != FDLP_OK) return rc;
  const int kind = b->preprocess == FDLP_PRE_DIFF ? 2 : b->pcm_kind;
  HIP_TRY(fdlp::launch_mel(p->mc, p->frames.dev, nf, b->pcm_dev, kind, b->noise_dev, b->out_dev, b->out_f64_dev,
                           b->ark_decimals, s));
  return FDLP_OK;
}

// ---------------------------------------------------------------------------------------------
// MFCC plan (computeMfccFeatures.py:58-135, fdlp_mfcc.hip)
// ---------------------------------------------------------------------------------------------
struct fdlp_mfcc_plan {
  fdlp_mfcc_config cfg{};
  int device = 0;
  FrameGrid grid;
  int n = 0, nb = 0, K = 0, Kpad = 0, nbpad = 0, ncep = 0, width = 0, rt = 0;
  std::vector<double> fold, tw, dct;  // host copies (fdlp_mfcc_plan_tables)
  fdlp::MfccConsts mc{};
  double *d_win = nullptr, *d_fold = nullptr, *d_tw = nullptr, *d_dct = nullptr, *d_cep = nullptr;
  int *d_lo = nullptr, *d_hi = nullptr;
  Staging<fdlp::MfccFrame> frames;
  DeviceResources res;
};

int fdlp_mfcc_plan_create(const fdlp_mfcc_config* cfg, int device, fdlp_mfcc_plan** out) {
  if (!cfg || !out) return fail(FDLP_E_INVALID, "fdlp_mfcc_plan_create: null argument");
  *out = nullptr;
  const fdlp_mfcc_config& c = *cfg;
  if (c.nfilters < 1 || c.srate < 1 || c.frate < 1 || !(c.fduration > 0) || c.max_frames < 1 || c.context < 0)
    return fail(FDLP_E_INVALID, "invalid mfcc configuration");
  if (c.nfft < 2 || c.nfft % 2 || c.nfft > 65536) return fail(FDLP_E_INVALID, "nfft must be even and <= 65536");
  PlanPtr<fdlp_mfcc_plan> p(new (std::nothrow) fdlp_mfcc_plan);
  if (!p) return fail(FDLP_E_NOMEM, "out of memory");
  p->cfg = c;
  p->device = p->res.device = device;
  p->grid = FrameGrid(c.srate, c.fduration, (int)((double)c.srate / (double)c.frate));  // features.py:135
  const int L = p->grid.L;
  if (L < 2 || p->grid.hop < 1) return fail(FDLP_E_INVALID, "frame length / hop too small");
  const int n = c.nfft / 2 + 1;  // fft(time_frames, int(nfft / 2 + 1))                  (:126)
  const int nb = n / 2 + 1;      // real input: bins n-k mirror bins k
  const int K = std::min(L, n);
  p->n = n; p->nb = nb; p->K = K;
  p->Kpad = (K + 3) / 4 * 4;
  p->nbpad = (nb + 15) / 16 * 16;
  p->ncep = std::min(13, c.nfilters);  // dct(...)[:, 0:13]                              (:127-128)
  p->width = p->ncep * (2 * c.context + 1);
  p->rt = fdlp::mfcc_row_tiles(p->Kpad, p->nbpad, c.nfilters);
  if (p->rt == 0)
    return fail(FDLP_E_INVALID, "mfcc tile exceeds the 160 KB LDS: need max(min(L, n), nfilters) + n/2 <= ~1230 "
                                "(n = nfft/2 + 1, L = srate * fduration)");
  int ncol = 0;
  const std::vector<double> fb = fbank_mel(c.nfilters, c.nfft, c.srate, 1.0, &ncol);  // createFbank   (:74)
  if (ncol != n) return fail(FDLP_E_INVALID, "filterbank width does not match nfft/2+1");
  // |X[n-k]| = |X[k]|: the mirrored columns fold onto bins 1 .. nb-1 (not onto the Nyquist bin of an even n)
  p->fold.assign((size_t)c.nfilters * nb, 0.0);
  for (int m = 0; m < c.nfilters; ++m)
    for (int k = 0; k < nb; ++k) {
      double v = fb[(size_t)m * n + k];
      if (k >= 1 && n - k != k) v += fb[(size_t)m * n + (n - k)];
      p->fold[(size_t)m * nb + k] = v;
    }
  std::vector<int> lo(c.nfilters, 0), hi(c.nfilters, 0);
  for (int m = 0; m < c.nfilters; ++m) band_support(&p->fold[(size_t)m * nb], nb, 0.0, &lo[m], &hi[m]);
  const std::vector<double> win = cos_window(L, 0.54, 0.46);  // np.hamming (:59)
  const long double PI = 3.141592653589793238462643383279502884L;
  // twiddles on the integer-reduced argument (i k) mod n, in long double
  const size_t ld = 2 * (size_t)p->nbpad;
  p->tw.assign((size_t)p->Kpad * ld, 0.0);
  for (int i = 0; i < K; ++i)
    for (int k = 0; k < nb; ++k) {
      const int64_t r = ((int64_t)i * k) % n;
      const long double ang = 2.0L * PI * (long double)r / (long double)n;
      p->tw[(size_t)i * ld + k] = (double)cosl(ang);
      p->tw[(size_t)i * ld + p->nbpad + k] = (double)-sinl(ang);
    }
  // scipy.fftpack.dct type 2, unnormalised: y[q] = 2 sum_m x[m] cos(pi q (2m+1) / (2 N))
  p->dct.assign((size_t)c.nfilters * p->ncep, 0.0);
  for (int m = 0; m < c.nfilters; ++m)
    for (int q = 0; q < p->ncep; ++q) {
      const int64_t r = ((int64_t)q * (2 * m + 1)) % (4 * (int64_t)c.nfilters);
      p->dct[(size_t)m * p->ncep + q] = (double)(2.0L * cosl(PI * (long double)r / (long double)(2 * c.nfilters)));
    }
  if (device < 0) {
    *out = p.release();
    return FDLP_OK;
  }
  std::optional<DeviceGuard> dg;
  int rc;
  if ((rc = open_device(device, dg)) != FDLP_OK) return rc;
  DeviceResources& res = p->res;
  if ((rc = upload(res, &p->d_win, win.data(), win.size())) != FDLP_OK) return rc;
  if ((rc = upload(res, &p->d_fold, p->fold.data(), p->fold.size())) != FDLP_OK) return rc;
  if ((rc = upload(res, &p->d_tw, p->tw.data(), p->tw.size())) != FDLP_OK) return rc;
  if ((rc = upload(res, &p->d_dct, p->dct.data(), p->dct.size())) != FDLP_OK) return rc;
  if ((rc = upload(res, &p->d_lo, lo.data(), lo.size())) != FDLP_OK) return rc;
  if ((rc = upload(res, &p->d_hi, hi.data(), hi.size())) != FDLP_OK) return rc;
  if (p->frames.arrays(res, (size_t)c.max_frames) != hipSuccess ||
      (c.context > 0 && res.device_array(&p->d_cep, (size_t)c.max_frames * p->ncep) != hipSuccess) ||
      p->frames.event(res) != hipSuccess)
    return fail(FDLP_E_NOMEM, "mfcc plan workspace allocation failed");
  fdlp::MfccConsts& m = p->mc;
  m.L = L; m.hop = p->grid.hop; m.ext = p->grid.ext; m.n = n; m.nb = nb; m.K = K; m.Kpad = p->Kpad;
  m.nbpad = p->nbpad;
  m.nfilters = c.nfilters; m.ncep = p->ncep; m.context = c.context; m.rt = p->rt;
  m.window = p->d_win; m.tw = p->d_tw; m.fold = p->d_fold; m.lo = p->d_lo; m.hi = p->d_hi; m.dct = p->d_dct;
  *out = p.release();
  return FDLP_OK;
}

int fdlp_mfcc_plan_destroy(fdlp_mfcc_plan* p) { delete p; return FDLP_OK; }

int fdlp_mfcc_geometry(const fdlp_mfcc_plan* p, int64_t T, int32_t* F, int32_t* width) {
  if (!p || !F || T < 0) return fail(FDLP_E_INVALID, "fdlp_mfcc_geometry: bad args");
  *F = (int32_t)p->grid.frames_of(T);
  if (width) *width = p->width;
  return FDLP_OK;
}

int fdlp_mfcc_plan_tables(const fdlp_mfcc_plan* p, int32_t* dims, double* fold, double* tw, double* dct) {
  if (!p || !dims) return fail(FDLP_E_INVALID, "fdlp_mfcc_plan_tables: bad args");
  const int32_t d[8] = {p->n, p->nb, p->K, p->Kpad, p->nbpad, p->ncep, p->cfg.nfilters, 16 * p->rt};
  memcpy(dims, d, sizeof(d));
  if (fold) memcpy(fold, p->fold.data(), sizeof(double) * p->fold.size());
  if (tw) memcpy(tw, p->tw.data(), sizeof(double) * p->tw.size());
  if (dct) memcpy(dct, p->dct.data(), sizeof(double) * p->dct.size());
  return FDLP_OK;
}

int fdlp_mfcc_compute(fdlp_mfcc_plan* p, const fdlp_batch* b, void* stream) {
  if (!p || !b || p->device < 0) return fail(FDLP_E_INVALID, "fdlp_mfcc_compute: bad args or host-only plan");
  if (b->n_utt < 0 || (b->n_utt > 0 && (!b->pcm_dev || !b->pcm_off || !b->utt_len || !b->out_row)) ||
      (!b->out_dev && !b->out_f64_dev))
    return fail(FDLP_E_INVALID, "fdlp_mfcc_compute: bad batch");
  if (b->pcm_kind != FDLP_PCM_I16 && b->pcm_kind != FDLP_PCM_F64) return fail(FDLP_E_INVALID, "unknown pcm_kind");
  if (b->noise_dev && (!b->noise_off || !b->noise_alpha || b->pcm_kind != FDLP_PCM_I16))
    return fail(FDLP_E_INVALID, "noise mixing needs int16 PCM and the noise arrays");
  if (b->preprocess != FDLP_PRE_NONE) return fail(FDLP_E_INVALID, "computeMfccFeatures.py has no diff preprocessing");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard dg(p->device);  // the caller's current device is restored on return
  HIP_TRY(dg.status());
  int rc;
  if ((rc = p->frames.wait()) != FDLP_OK) return rc;
  int nf = 0;
  for (int u = 0; u < b->n_utt; ++u) {
    const int64_t T = b->utt_len[u];
    if (T < 1 || T > INT32_MAX || b->pcm_off[u] < 0) return fail(FDLP_E_INVALID, "empty or oversized utterance");
    const int64_t F = p->grid.frames_of(T);
    if (nf + F > p->cfg.max_frames) return fail(FDLP_E_CAPACITY, "batch exceeds the mfcc plan's max_frames");
    fill_frames(p->frames.host + nf, b, u, T, F, [F](fdlp::MfccFrame& fd) {
      fd.F = (int32_t)F;
      fd.pad_ = 0;
    });
    nf += (int)F;
  }
  if (nf == 0) return FDLP_OK;
  if ((rc = p->frames.publish((size_t)nf, s)) != FDLP_OK) return rc;
  HIP_TRY(fdlp::launch_mfcc(p->mc, p->frames.dev, nf, b->pcm_dev, b->pcm_kind, b->noise_dev, p->d_cep, b->out_dev,
                            b->out_f64_dev, b->ark_decimals, s));
  return FDLP_OK;
}
