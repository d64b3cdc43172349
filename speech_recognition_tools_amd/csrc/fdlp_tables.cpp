// fdlp_tables.cpp -- the host table builders of the plans: numpy's linspace and windows, the filterbanks
// (features.py:172-219), the structured-autocorrelation tables, the DFT splits, the gamma weights, DeltaFeatures'
// scales and the OLA slices (computeFDLPSpectrogram.py:207-225).  No HIP call.
#include <thread>

#include "fdlp_plan_common.h"

namespace fdlp {
namespace host {

// numpy.linspace(start, stop, num): i*step + start, last element = stop exactly.
std::vector<double> linspace(double start, double stop, int num) {
  std::vector<double> y(num);
  if (num == 1) { y[0] = start; return y; }
  const double step = (stop - start) / (double)(num - 1);
  for (int i = 0; i < num; ++i) y[i] = (double)i * step + start;
  if (num > 1) y[num - 1] = stop;
  return y;
}

// numpy.hamming / numpy.hanning: c0 + c1*cos(pi*n/(M-1)), n = 1-M, 3-M, ..., M-1
std::vector<double> cos_window(int M, double c0, double c1) {
  std::vector<double> w(std::max(M, 0));
  if (M == 1) { w[0] = 1.0; return w; }
  for (int i = 0; i < M; ++i) {
    const double n = (double)(1 - M + 2 * i);
    w[i] = c0 + c1 * cos(M_PI * n / (double)(M - 1));
  }
  return w;
}

// createFbankCochlear (features.py:193-219)
std::vector<double> fbank_cochlear(int nf, int nfft, int srate, double om_w, double alp, int fixed, double bet,
                                   double wf, int* ncol_out) {
  auto bark = [wf](double x) { return 6.0 * asinh((x / wf) / 600.0); };
  const double fmax = (double)srate / 2.0;
  const std::vector<double> cf = linspace(0.0, bark(fmax), nf);
  const int ncol = (int)floor((double)nfft / 2.0 + 1.0);
  std::vector<double> fl = linspace(0.0, fmax, ncol);
  for (auto& v : fl) v = bark(v);
  std::vector<double> W((size_t)nf * ncol);
  auto rows = [&](int i0, int i1) {
    for (int i = i0; i < i1; ++i) {
      const double fc = cf[i];
      const double a = fixed == 1 ? alp : alp * exp(-0.1 * fc);
      for (int j = 0; j < ncol; ++j) {
        const double d = fl[j] - fc;
        double v;
        if (d <= -om_w / 2.0) v = pow(10.0, a * (d + om_w / 2.0));
        else if (d > -om_w / 2.0 && d < om_w / 2.0) v = 1.0;
        else v = pow(10.0, -bet * (d - om_w / 2.0));
        W[(size_t)i * ncol + j] = v;
      }
    }
  };
  // ~2M pow calls for the recipes' 80 x 24001 taps: rows on a few threads (same values per element)
  const int nt = std::max(1, std::min({8, nf, (int)std::thread::hardware_concurrency()}));
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) th.emplace_back(rows, nf * t / nt, nf * (t + 1) / nt);
  rows(0, nf / nt);
  for (auto& x : th) x.join();
  *ncol_out = ncol;
  return W;
}

// createFbank (features.py:172-190)
std::vector<double> fbank_mel(int nf, int nfft, int srate, double wf, int* ncol_out) {
  const double mel_max = 2595.0 * log10(1.0 + ((double)srate / wf) / 1400.0);
  const std::vector<double> mels = linspace(0.0, mel_max, nf + 2);
  const int ncol = (int)floor((double)nfft / 2.0 + 1.0);
  std::vector<double> edge(nf + 2);
  for (int i = 0; i < nf + 2; ++i) {
    const double hz = wf * (700.0 * (pow(10.0, mels[i] / 2595.0) - 1.0));
    edge[i] = floor((double)(nfft + 1) * hz / (double)srate);
  }
  std::vector<double> W((size_t)nf * ncol, 0.0);
  for (int m = 1; m <= nf; ++m) {
    const int l = (int)edge[m - 1], c = (int)edge[m], r = (int)edge[m + 1];
    for (int k = l; k < c; ++k)
      if (k >= 0 && k < ncol) W[(size_t)(m - 1) * ncol + k] = ((double)k - edge[m - 1]) / (edge[m] - edge[m - 1]);
    for (int k = c; k < r; ++k)
      if (k >= 0 && k < ncol) W[(size_t)(m - 1) * ncol + k] = (edge[m + 1] - (double)k) / (edge[m + 1] - edge[m]);
  }
  *ncol_out = ncol;
  return W;
}

// Split the flat sweep [fl_lo, fl_hi) into H parts of equal work (more waves: the flat sweep has one unit
// per frame against two for the skirts): a position costs 1, an event (restart or emission: the fold into
// every chain, the masked extra pass of the block it splits) kFlatEventCost positions -- fitted to the
// recipes' sweep (A = 10 lags per lane, C = 5 chains) from per-wave timings, where equal position parts
// ran 858 / 1067 us (median) with 34 / 126 events.  Part h covers [P_{h+1}, P_h) and takes
// the events with P_{h+1} <= S < P_h (part 0 also S = fl_hi).  Band j needs the partial chain of part h
// when its flat top crosses the part's lower end: m1_j < P_{h+1} < m2_j.
static constexpr double kFlatEventCost = 35.0;
static void flat_parts(SkirtTables* T, int B, int H) {
  if (T->fl_hi - T->fl_lo < 1024 * H) H = 1;
  T->fl_H = H;
  std::vector<int> P(H + 1);
  {
    // cost above position n (sweep order: top down), then the cut points at h / H of the total
    const int lo = T->fl_lo, hi = T->fl_hi, len = hi - lo;
    std::vector<double> above(len + 1, 0.0);  // above[i]: cost of positions [hi - i, hi) and their events
    std::vector<int> ev_at(len + 1, 0);
    for (const auto& e : T->fl) ev_at[std::min(std::max(hi - e.S, 0), len)] += 1;
    for (int i = 1; i <= len; ++i) above[i] = above[i - 1] + 1.0 + kFlatEventCost * ev_at[i];
    P[0] = hi;
    P[H] = lo;
    for (int h = 1, i = 0; h < H; ++h) {
      const double target = above[len] * h / H;
      while (i < len && above[i] < target) ++i;
      P[h] = hi - i;
    }
  }
  for (int h = 0; h < H; ++h) { T->part_hi[h] = P[h]; T->part_lo[h] = P[h + 1]; }
  const int nev = (int)T->fl.size();
  T->part_ev[0] = 0;
  for (int h = 1; h <= H; ++h) {
    int k = T->part_ev[h - 1];
    if (h == H) k = nev;
    else while (k < nev && T->fl[k].S >= P[h]) ++k;
    T->part_ev[h] = k;
  }
  T->fl_band.assign(B, make_int2(0, 0));
  for (int j = 0; j < B; ++j) {
    int mask = 0;
    for (int h = 0; h + 1 < H; ++h)
      if (T->reg[j].x < P[h + 1] && P[h + 1] < T->reg[j].y) mask |= 1 << h;
    T->fl_band[j] = make_int2(j % std::max(T->fl_C, 1), mask);
  }
}

// Events of the flat-top sweep: band j restarts chain j mod C at m2_j and emits it at m1_j.  Order:
// S descending; at equal S bands descending (band j emits before band j - C restarts) and a band's
// restart before its own emission.  C is the smallest count for which no chain is restarted while
// it still serves a band (checked by replaying the events).
static void flat_events(SkirtTables* T, int B) {
  T->fl_C = 0;
  T->fl.clear();
  T->fl_lo = INT32_MAX;
  T->fl_hi = 0;
  for (int j = 0; j < B; ++j) {
    T->fl_lo = std::min(T->fl_lo, T->reg[j].x);
    T->fl_hi = std::max(T->fl_hi, T->reg[j].y);
  }
  for (int C = 1; C <= 8; ++C) {
    std::vector<FlatEv> ev;
    for (int j = 0; j < B; ++j) {
      ev.push_back(FlatEv{T->reg[j].y, j, 0, j % C});
      ev.push_back(FlatEv{T->reg[j].x, j, 1, j % C});
    }
    std::sort(ev.begin(), ev.end(), [](const FlatEv& a, const FlatEv& b) {
      if (a.S != b.S) return a.S > b.S;
      if (a.band != b.band) return a.band > b.band;
      return a.type < b.type;
    });
    std::vector<int> owner(C, -1);
    bool ok = true;
    for (const auto& e : ev) {
      if (e.type == 0) {
        if (owner[e.chain] != -1) { ok = false; break; }
        owner[e.chain] = e.band;
      } else {
        if (owner[e.chain] != e.band) { ok = false; break; }
        owner[e.chain] = -1;
      }
    }
    if (ok) {
      T->fl = ev;
      T->fl_C = C;
      flat_parts(T, B, 2);  // two position parts (3 and 4 measured slower)
      return;
    }
  }
}

bool skirt_tables(const fdlp_config& c, int B, int N, int nfft, SkirtTables* T) {
  if (c.fbank_kind != FDLP_FBANK_COCHLEAR || c.fixed != 1) return false;
  const double wf = c.warp_fact, om = c.om_w, a = c.alp, b = c.bet;
  if (!std::isfinite(wf) || !std::isfinite(om) || !std::isfinite(a) || !std::isfinite(b)) return false;
  auto bark = [wf](double x) { return 6.0 * asinh((x / wf) / 600.0); };
  const double fmax = (double)c.srate / 2.0;
  const std::vector<double> cf = linspace(0.0, bark(fmax), B);
  const int ncol = (int)floor((double)nfft / 2.0 + 1.0);
  if (ncol - 1 != N) return false;
  std::vector<double> fl = linspace(0.0, fmax, ncol);
  for (auto& v : fl) v = bark(v);
  T->reg.resize(B);
  for (int j = 0; j < B; ++j) {
    int state = 0, m1 = 0, m2 = 0;
    for (int m = 0; m < N; ++m) {
      const double d = fl[m] - cf[j];
      const int cls = d <= -om / 2.0 ? 0 : ((d > -om / 2.0 && d < om / 2.0) ? 1 : 2);
      if (cls < state) return false;
      state = cls;
      if (cls == 0) m1 = m + 1;
      if (cls <= 1) m2 = m + 1;
    }
    if (m2 < m1) m2 = m1;
    T->reg[j] = make_int2(m1, m2);
  }
  const long double c0 = 0.5L * ((long double)fl[0] + (long double)fl[N - 1]);
  const long double span = std::max(fabsl((long double)fl[N - 1] - c0), fabsl((long double)fl[0] - c0));
  if (fabsl((long double)a) * span > 60.0L || fabsl((long double)b) * span > 60.0L) return false;
  T->e.resize(2 * (size_t)N);
  for (int m = 0; m < N; ++m) {
    const long double x = (long double)fl[m] - c0;
    T->e[m] = (double)powl(10.0L, (long double)a * x);
    T->e[(size_t)N + m] = (double)powl(10.0L, -(long double)b * x);
  }
  std::vector<double> K(2 * (size_t)B);
  for (int j = 0; j < B; ++j) {
    const long double ea = (long double)a * ((long double)om - 2.0L * cf[j] + 2.0L * c0);
    const long double eb = (long double)b * (2.0L * cf[j] + (long double)om - 2.0L * c0);
    if (fabsl(ea) > 150.0L || fabsl(eb) > 150.0L) return false;
    K[j] = (double)powl(10.0L, ea);
    K[(size_t)B + j] = (double)powl(10.0L, eb);
  }
  const int L1 = c.order + 1;  // nlags - 1: the longest straddle
  T->wrap_kw.assign(B, 0.0);
  T->wrap_any = false;
  for (int j = 0; j < B; ++j) {
    if (T->reg[j].x >= L1 && T->reg[j].y <= N - L1) {
      const long double ea = (long double)a * ((long double)om - 2.0L * cf[j] + 2.0L * c0);
      const long double eb = (long double)b * (2.0L * cf[j] + (long double)om - 2.0L * c0);
      T->wrap_kw[j] = (double)powl(10.0L, 0.5L * (ea + eb));
      T->wrap_any = true;
    }
  }
  T->snap.resize(2 * (size_t)B);
  for (int sk = 0; sk < 2; ++sk) {
    std::vector<SkSnap> t(B);
    for (int j = 0; j < B; ++j)
      t[j] = SkSnap{sk == 0 ? N - T->reg[j].x : T->reg[j].y, j, K[(size_t)sk * B + j]};
    std::stable_sort(t.begin(), t.end(), [](const SkSnap& u, const SkSnap& v) { return u.S > v.S; });
    for (int j = 0; j < B; ++j) T->snap[(size_t)sk * B + j] = t[j];
    T->smin[sk] = t[B - 1].S;
  }
  flat_events(T, B);
  return true;
}

// radix split of n over the supported radices (4s first, then 2, 3, 5, 7)
bool factor_radices(int n, DftPlan* d) {
  d->n = n;
  d->nrad = 0;
  int m = n;
  auto push = [d](int r) {
    if (d->nrad >= kMaxRadices) return false;
    d->rad[d->nrad++] = r;
    return true;
  };
  while (m % 4 == 0) { if (!push(4)) return false; m /= 4; }
  while (m % 2 == 0) { if (!push(2)) return false; m /= 2; }
  for (int r : {3, 5, 7})
    while (m % r == 0) { if (!push(r)) return false; m /= r; }
  return m == 1;
}

// split N = N1 * N2 with both sub-DFTs LDS-resident, N1 ~ sqrt(N)
bool split_four_step(int N, DftPlan* d1, DftPlan* d2) {
  int best = -1;
  for (int n1 = 1; n1 <= N; ++n1) {
    if (N % n1) continue;
    const int n2 = N / n1;
    if (n1 > kDftMaxSub || n2 > kDftMaxSub) continue;
    DftPlan a, b;
    if (!factor_radices(n1, &a) || !factor_radices(n2, &b)) continue;
    if (best < 0 || std::abs(n1 - n2) < std::abs(best - N / best)) best = n1;
  }
  if (best < 0) return false;
  factor_radices(best, d1);
  factor_radices(N / best, d2);
  return true;
}

double gamma_pdf(double x, double a, double loc, double scale) {
  // scipy.stats.gamma.pdf = exp(xlogy(a-1, y) - y - gammaln(a)) / scale, y = (x-loc)/scale >= 0
  const double y = (x - loc) / scale;
  if (!(y >= 0.0)) return 0.0;
  const double xl = (a - 1.0 == 0.0) ? 0.0 : (a - 1.0) * log(y);
  return exp(xl - y - lgamma(a)) / scale;
}

// DeltaFeatures' scale tables.  scales[i] = scales[i-1] convolved with j = -window .. window, over sum j^2: the
// numerators are integers (exact in double), the denominator is (sum j^2)^i, one rounding to float32.
void post_scale_tables(int order, int window, std::vector<int32_t>& lens, std::vector<float>& flat) {
  std::vector<double> prev{1.0};
  double denom = 1.0, norm = 0.0;
  for (int j = -window; j <= window; ++j) norm += (double)j * j;
  lens.assign(1, 1);
  flat.assign(1, 1.0f);
  for (int i = 1; i <= order; ++i) {
    const int po = ((int)prev.size() - 1) / 2, co = po + window;
    std::vector<double> cur(prev.size() + 2 * (size_t)window, 0.0);
    for (int j = -window; j <= window; ++j)
      for (int k = -po; k <= po; ++k) cur[(size_t)(j + k + co)] += (double)j * prev[(size_t)(k + po)];
    denom *= norm;
    lens.push_back((int32_t)cur.size());
    for (double v : cur) flat.push_back((float)(v / denom));
    prev.swap(cur);
  }
}

// OLA slices of computeFDLPSpectrogram.py:207-225 (see oracle.ola_plan for the numpy rules)
int ola_table(int kk, int kkb2, int ola_hop, int F, int L, const uint8_t* jit, int32_t* dst, int32_t* src,
              int32_t* cnt) {
  int64_t ptr = 0;
  for (int i = 0; i < F; ++i) {
    if (i == 0) {
      if (L < kkb2) {
        const int rhs = std::max(0, std::min(L, kk - kkb2));
        if (rhs != L) return fail(FDLP_E_BROADCAST, "reference OLA would fail to broadcast (frame 0)");
        dst[i] = 0; src[i] = kkb2; cnt[i] = L;
      } else {
        if (kk - kkb2 != kkb2) return fail(FDLP_E_BROADCAST, "reference OLA would fail to broadcast (frame 0)");
        dst[i] = 0; src[i] = kkb2; cnt[i] = kkb2;
      }
    } else if (i == F - 1 || i == F - 2) {
      const int64_t n = (int64_t)L - ptr;
      if (kk >= n) {
        const int64_t lhs = std::max<int64_t>(0, n);
        const int64_t rhs = n >= 0 ? n : std::max<int64_t>(0, kk + n);
        if (lhs != rhs) return fail(FDLP_E_BROADCAST, "reference OLA would fail to broadcast (tail frame)");
        dst[i] = (int32_t)ptr; src[i] = 0; cnt[i] = (int32_t)lhs;
      } else {
        dst[i] = (int32_t)ptr; src[i] = 0; cnt[i] = kk;
      }
    } else {
      if (ptr + kk > L) return fail(FDLP_E_BROADCAST, "reference OLA would fail to broadcast (middle frame)");
      dst[i] = (int32_t)ptr; src[i] = 0; cnt[i] = kk;
    }
    if (i == 0) ptr = ptr + ola_hop - kkb2;
    else ptr = ptr + ola_hop + (jit ? jit[i - 1] : 0);
  }
  return FDLP_OK;
}

}  // namespace host
}  // namespace fdlp
