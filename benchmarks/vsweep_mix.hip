// Microbenchmark: instruction mixes of ac_vsweep_kernel's inner block on gfx950 (one wave = 4 units of
// 16 lanes; per block 100 fp64 FMAs per lane into 10 accumulators).
//   fma   : broadcasts from registers (no DPP), window in registers
//   dpp   : 10 row_newbcast broadcasts per block (bound_ctrl), window in registers
//   lds   : dpp + the window's A new values and cur read from an LDS ring each block (two banks)
//   ldsdpp / ldsrev / ldsrev0 / ldsrevc : the kernel's own block (v_fmac_f64_dpp broadcasts,
//           window reads at the block head) in two FMA orders, see krev below
//   fc22 (argument "fc"): the ldsrev block in the 2x2 fast-correlation form, 75 FMAs per block, see k22 below
//   kx modes (argument "ctl"): ldsrev plus the kernel's per-block control flow, see kx below
// The ring rows are 544 doubles, the kernel's conflict-free stride.
// Build: hipcc -O3 --offload-arch=gfx950 benchmarks/vsweep_mix.hip -o benchmarks/vsweep_mix
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>

constexpr int A = 10;
template <int K>
__device__ __forceinline__ double bc(double v) { return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + K, 0xF, 0xF, true); }
template <int V = 0>
__device__ __forceinline__ void bcast_all(double (&bb)[A], double cur) {
  if constexpr (V < A) { bb[V] = bc<V>(cur); bcast_all<V + 1>(bb, cur); }
}
__device__ __forceinline__ void block(double (&acc)[A], const double (&bb)[A], const double (&lo)[A], const double (&hi)[A]) {
#pragma unroll
  for (int v = 0; v < A; ++v)
#pragma unroll
    for (int u = 0; u < A; ++u) acc[u] = fma(bb[v], (v + u < A) ? lo[v + u] : hi[v + u - A], acc[u]);
}

template <int MODE>
__global__ __launch_bounds__(64, 2) void k(const double* in, double* out, int iters) {
  __shared__ double ring[4][544];
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  for (int q = l; q < 544; q += 16) ring[row][q] = in[(q + row) & 255] + 1e-3 * q;
  __syncthreads();
  double acc[A], X[A], Y[A], bb[A];
  for (int u = 0; u < A; ++u) { acc[u] = 0; X[u] = in[u + l]; Y[u] = in[u + 20 + l]; bb[u] = in[u + 40]; }
  double cur = in[l];
  for (int it = 0; it < iters; ++it) {
    const int n0 = (it * 2 * A) & 511;
    if constexpr (MODE == 2) {
      const int base = (n0 + A * l) & 510;
#pragma unroll
      for (int q = 0; q < A; ++q) X[q] = ring[row][base + q];
      cur = ring[row][(n0 + l) & 511];
    }
    if constexpr (MODE >= 1) bcast_all(bb, cur); else { cur = cur * 0.9999; bb[0] = cur; }
    block(acc, bb, X, Y);
    if constexpr (MODE == 2) {
      const int base = (n0 + A + A * l) & 510;
#pragma unroll
      for (int q = 0; q < A; ++q) Y[q] = ring[row][base + q];
      cur = ring[row][(n0 + A + l) & 511];
    }
    if constexpr (MODE >= 1) bcast_all(bb, cur); else { cur = cur * 0.9999; bb[1] = cur; }
    block(acc, bb, Y, X);
  }
  double s = 0;
  for (int u = 0; u < A; ++u) s += acc[u];
  out[blockIdx.x * 64 + threadIdx.x] = s;
}

// ldspf: as lds, but each block's window (and broadcast source) is read one block ahead into a third
// register bank, so the wait at a block head is for reads issued a whole block earlier
__global__ __launch_bounds__(64, 2) void kpf(const double* in, double* out, int iters) {
  __shared__ double ring[4][544];
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  for (int q = l; q < 544; q += 16) ring[row][q] = in[(q + row) & 255] + 1e-3 * q;
  __syncthreads();
  double acc[A], B0[A], B1[A], B2[A], bb[A];
  for (int u = 0; u < A; ++u) { acc[u] = 0; B0[u] = in[u + l]; B2[u] = in[u + 20 + l]; bb[u] = in[u + 40]; }
  double cur = in[l], curn;
  auto rd = [&](double (&dst)[A], double& c, int n0) {
    const int base = (n0 + A * l) & 510;
#pragma unroll
    for (int q = 0; q < A; ++q) dst[q] = ring[row][base + q];
    c = ring[row][(n0 + l) & 511];
  };
  for (int it = 0; it < iters; it += 3) {
    const int n0 = (it * A) & 511;
    rd(B1, curn, n0 + A);
    bcast_all(bb, cur);
    block(acc, bb, B0, B2);
    cur = curn;
    rd(B2, curn, n0 + 2 * A);
    bcast_all(bb, cur);
    block(acc, bb, B1, B0);
    cur = curn;
    rd(B0, curn, n0 + 3 * A);
    bcast_all(bb, cur);
    block(acc, bb, B2, B1);
    cur = curn;
  }
  double s = 0;
  for (int u = 0; u < A; ++u) s += acc[u];
  out[blockIdx.x * 64 + threadIdx.x] = s;
}

// dppwin: the window moves one lane down per block by DPP (row_shr:1, two v_mov_b32_dpp per double); only
// lane 0 of each row reads its 10 new values (and the broadcast source) from the LDS ring
template <int SH = 0>
__device__ __forceinline__ void shift_in(double (&dst)[A], const double (&src)[A], const double (&nv)[A]) {
#pragma unroll
  for (int q = 0; q < A; ++q) dst[q] = __builtin_amdgcn_update_dpp(nv[q], src[q], 0x111, 0xF, 0xF, false);
}
__global__ __launch_bounds__(64, 2) void kdw(const double* in, double* out, int iters) {
  __shared__ double ring[4][544];
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  for (int q = l; q < 544; q += 16) ring[row][q] = in[(q + row) & 255] + 1e-3 * q;
  __syncthreads();
  double acc[A], X[A], Y[A], bb[A], nv[A];
  for (int u = 0; u < A; ++u) { acc[u] = 0; X[u] = in[u + l]; Y[u] = in[u + 20 + l]; bb[u] = in[u + 40]; nv[u] = 0; }
  double cur = in[l];
  for (int it = 0; it < iters; ++it) {
    const int n0 = (it * 2 * A) & 511;
    if (l == 0) {
#pragma unroll
      for (int q = 0; q < A; ++q) nv[q] = ring[row][(n0 + q) & 510];
    }
    cur = ring[row][(n0 + l) & 511];
    shift_in(Y, X, nv);  // new lo (Y) from the old lo (X) of the lane below; X becomes hi
    bcast_all(bb, cur);
    block(acc, bb, Y, X);
    if (l == 0) {
#pragma unroll
      for (int q = 0; q < A; ++q) nv[q] = ring[row][(n0 + A + q) & 510];
    }
    cur = ring[row][(n0 + A + l) & 511];
    shift_in(X, Y, nv);
    bcast_all(bb, cur);
    block(acc, bb, X, Y);
  }
  double s = 0;
  for (int u = 0; u < A; ++u) s += acc[u];
  out[blockIdx.x * 64 + threadIdx.x] = s;
}

// krev: the block as ac_vsweep_kernel issues it (one v_fmac_f64_dpp per product, the ten window reads at
// the block head; the compiler emits them in address order, lo[0:1] first) with the FMAs in one of two orders:
//   ORDER 0  rows v = 0..A-1, u fastest: the first FMA reads lo[0], a value that was just read
//   ORDER 1  the 45 products of the previous block's bank first (by window element, so consecutive FMAs
//            write distinct accumulators), then the new bank by window element from lo[0] up, the order in
//            which the reads return: the partial lgkmcnt waits release them pair by pair
// STRICT: the FMAs are volatile and keep that order (ldsrev, ldsrev0).  Without it (ldsrevc) the scheduler
// spreads the new-bank products among the old-bank ones: 9 FMAs, the wait for lo[0:1], 18 FMAs, the wait
// for lo[2:3], and so on.
// AHEAD: cur (the DPP source) comes from a read issued one block earlier (2 more VGPRs); otherwise it is
// read in the block itself.
template <int V, bool STRICT>
__device__ __forceinline__ void fmac_bcast(double& acc, double cur, double w) {
  if constexpr (STRICT)
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(cur), "v"(w), "n"(V));
  else
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(cur), "v"(w), "n"(V));
}
struct Order { int v[A * A], u[A * A]; };
template <int ORDER>
constexpr Order make_order() {
  Order o{};
  int n = 0;
  if (ORDER == 0) {
    for (int v = 0; v < A; ++v)
      for (int u = 0; u < A; ++u) { o.v[n] = v; o.u[n] = u; ++n; }
    return o;
  }
  // old group w: the products with hi[w], u = A-1 .. w+1; new group q: the products with lo[q], u = q .. 0
  for (int w = 0; w < A - 1; ++w)
    for (int u = A - 1; u > w; --u) { o.v[n] = A + w - u; o.u[n] = u; ++n; }
  for (int q = 0; q < A; ++q)
    for (int u = q; u >= 0; --u) { o.v[n] = q - u; o.u[n] = u; ++n; }
  return o;
}
template <int ORDER, bool STRICT, int I = 0>
__device__ __forceinline__ void fma_seq(double (&acc)[A], double cm, const double (&lo)[A], const double (&hi)[A]) {
  if constexpr (I < A * A) {
    constexpr Order o = make_order<ORDER>();
    constexpr int v = o.v[I], u = o.u[I];
    fmac_bcast<v, STRICT>(acc[u], cm, (v + u < A) ? lo[v + u] : hi[v + u - A]);
    fma_seq<ORDER, STRICT, I + 1>(acc, cm, lo, hi);
  }
}
template <int ORDER, bool AHEAD, bool STRICT>
__global__ __launch_bounds__(64, 2) void krev(const double* in, double* out, int iters) {
  __shared__ double ring[4][544];
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  for (int q = l; q < 544; q += 16) ring[row][q] = in[(q + row) & 255] + 1e-3 * q;
  __syncthreads();
  double acc[A], X[A], Y[A];
  for (int u = 0; u < A; ++u) { acc[u] = 0; X[u] = in[u + l]; Y[u] = in[u + 20 + l]; }
  double cur = ring[row][l];
  auto blk = [&](int n0, double (&lo)[A], const double (&hi)[A]) {
    double c;
    if constexpr (!AHEAD) c = ring[row][(n0 + l) & 511];
    const int base = (n0 + A * l) & 510;
#pragma unroll
    for (int q = 0; q < A; ++q) lo[q] = ring[row][base + q];
    if constexpr (AHEAD) { c = cur; cur = ring[row][(n0 + A + l) & 511]; }
    double cm;
    asm volatile("v_mov_b64 %0, %1\n\ts_nop 1" : "=v"(cm) : "v"(c));
    fma_seq<ORDER, STRICT>(acc, cm, lo, hi);
  };
  for (int it = 0; it < iters; ++it) {
    const int n0 = (it * 2 * A) & 511;
    blk(n0, X, Y);
    blk(n0 + A, Y, X);
  }
  double s = 0;
  for (int u = 0; u < A; ++u) s += acc[u];
  out[blockIdx.x * 64 + threadIdx.x] = s;
}

// k22 (mode fc22): the ldsrev block in the 2x2 fast-correlation form.  For even v, u, with g0 = s[n0+v],
// g1 = s[n0+v+1] and W the lane's window,
//   Q[u]   += g0        * (W[v+u]   - W[v+u+1])
//   M[u/2] += (g0 + g1) *  W[v+u+1]
//   Q[u+1] += g1        * (W[v+u+2] - W[v+u+1])
// and acc[u] = Q[u] + M[u/2], acc[u+1] = Q[u+1] + M[u/2]: three products per 2 positions x 2 lags, 75 per
// block instead of 100, plus A subtractions and one addition.  Per bank the wave keeps the signed
// differences e[q] (even q: W[q] - W[q+1], odd q: W[q+1] - W[q]; e[A-1] crosses into the older bank), the raw
// odd elements and the raw W[0] (for the next block's e[A-1]); A is even, so the older bank's differences are
// reused as they are.  curs (lane v = s[n0+v] + s[n0+v+1]) is the second DPP source: one more ring read per
// block, issued a block ahead like cur's, and the addition.  Same ring row, same window reads, same FMA
// discipline as ldsrev (ordered v_fmac_f64_dpp, the 30 products of the older bank first, then the new bank by
// window element, consecutive FMAs on distinct accumulators).  M is folded into Q after the loop.
struct Bank22 { double e[A], od[A / 2], w0; };
constexpr int kN22 = 3 * (A / 2) * (A / 2);
struct Order22 { int src[kN22], v[kN22], acc[kN22], op[kN22], nold; };  // src 0: cur x e[op] -> Q[acc]; 1: curs x W[op] -> M[acc]
constexpr Order22 make_order22() {
  Order22 o{};
  int n = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int t = pass == 0 ? A : 0; t <= (pass == 0 ? 2 * A - 4 : A - 2); t += 2) {  // tiles with v + u = t
      const int umax = t < A - 2 ? t : A - 2, umin = t - (A - 2) > 0 ? t - (A - 2) : 0;
      for (int u = umax; u >= umin; u -= 2) { o.src[n] = 0; o.v[n] = t - u; o.acc[n] = u; o.op[n] = t; ++n; }
      for (int u = umax; u >= umin; u -= 2) { o.src[n] = 1; o.v[n] = t - u; o.acc[n] = u / 2; o.op[n] = t + 1; ++n; }
      for (int u = umax; u >= umin; u -= 2) { o.src[n] = 0; o.v[n] = t - u + 1; o.acc[n] = u + 1; o.op[n] = t + 1; ++n; }
    }
    if (pass == 0) o.nold = n;
  }
  return o;
}
template <int I, int END>
__device__ __forceinline__ void fma22(double (&Q)[A], double (&M)[A / 2], double cm, double csm, const Bank22& lo,
                                      const Bank22& hi) {
  if constexpr (I < END) {
    constexpr Order22 o = make_order22();
    constexpr int v = o.v[I], a = o.acc[I], op = o.op[I];
    if constexpr (o.src[I] == 0) fmac_bcast<v, true>(Q[a], cm, op < A ? lo.e[op] : hi.e[op - A]);
    else fmac_bcast<v, true>(M[a], csm, op < A ? lo.od[op / 2] : hi.od[(op - A) / 2]);
    fma22<I + 1, END>(Q, M, cm, csm, lo, hi);
  }
}
__global__ __launch_bounds__(64, 2) void k22(const double* in, double* out, int iters) {
  __shared__ double ring[4][544];
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  for (int q = l; q < 544; q += 16) ring[row][q] = in[(q + row) & 255] + 1e-3 * q;
  __syncthreads();
  double Q[A], M[A / 2];
  Bank22 X, Y;
  for (int u = 0; u < A; ++u) { Q[u] = 0; M[u / 2] = 0; X.e[u] = in[u + l]; Y.e[u] = in[u + 20 + l]; }
  for (int u = 0; u < A / 2; ++u) { X.od[u] = in[u + 40 + l]; Y.od[u] = in[u + 50 + l]; }
  X.w0 = in[60 + l]; Y.w0 = in[61 + l];
  double cur = ring[row][l], cur1 = ring[row][(1 + l) & 511];
  constexpr int kOld = make_order22().nold;
  static_assert(kOld == 3 * (A / 2) * (A / 2 - 1) / 2, "older-bank products");
  auto blk = [&](int n0, Bank22& lo, const Bank22& hi) {
    const int base = (n0 + A * l) & 510;
    double r[A];
#pragma unroll
    for (int q = 0; q < A; ++q) r[q] = ring[row][base + q];
    const double c = cur, cs = cur + cur1;
    cur = ring[row][(n0 + A + l) & 511];
    cur1 = ring[row][(n0 + A + 1 + l) & 511];
    double cm, csm;
    asm volatile("v_mov_b64 %0, %2\n\tv_mov_b64 %1, %3\n\ts_nop 1" : "=&v"(cm), "=&v"(csm) : "v"(c), "v"(cs));
    fma22<0, kOld>(Q, M, cm, csm, lo, hi);
    // the window is taken in behind the older bank's products
#pragma unroll
    for (int q = 0; q < A; ++q) asm volatile("" : "+v"(r[q]));
#pragma unroll
    for (int q = 0; q + 1 < A; ++q) lo.e[q] = (q & 1) ? r[q + 1] - r[q] : r[q] - r[q + 1];
    lo.e[A - 1] = hi.w0 - r[A - 1];
#pragma unroll
    for (int q = 0; q < A / 2; ++q) lo.od[q] = r[2 * q + 1];
    lo.w0 = r[0];
    fma22<kOld, kN22>(Q, M, cm, csm, lo, hi);
  };
  for (int it = 0; it < iters; ++it) {
    const int n0 = (it * 2 * A) & 511;
    blk(n0, X, Y);
    blk(n0 + A, Y, X);
  }
  double s = 0;
  for (int u = 0; u < A; ++u) s += Q[u] + M[u / 2];
  out[blockIdx.x * 64 + threadIdx.x] = s;
}

// kx: ldsrev (krev<1, true, true>) plus the per-block control flow that ac_vsweep_kernel's block carries and
// the microbenchmark's does not, one piece at a time.  Every test is wave-uniform and never true at run time
// (its operands are kernel arguments and table words, so the compiler keeps it); what is priced is the
// compare, the branch, and what their presence does to the waits and the schedule around them.
//   X_BR1  if (n >= ev) { handler }  ahead of the block: the kernel's `while (evS >= hi_m)`; the handler
//          stores an accumulator row and takes the next record
//   X_BR2  also if (n >= lim) { handler }: the kernel's ensure(); the handler writes the ring, as commit does
//   X_SEL  cur = (pos >= lo_m && pos < hi_m) ? cur : 0 with lo_m, hi_m as the kernel builds them
//   X_SLD  a four-word record requested by a scalar load in every block and taken in (asm "s" use) at the
//          head of the next, ahead of its ring reads, as the kernel takes nx in
//   X_ALL  BR1 + BR2 + SEL with the record requested in BR1's handler only and taken in at every block head:
//          the kernel's shape (the wait at the head is then the compiler's, for a load that may be pending)
//   R > 0  schedule walk: an outer loop does X_ALL's tests and takes one record in (requested one record
//          ahead); the record's second word is the count of (X, Y) block pairs that the inner loop then runs
//          with nothing but the blocks.  iters is still the total number of pairs.
typedef int Rec4 __attribute__((ext_vector_type(4), aligned(4)));
constexpr int X_BR1 = 1, X_BR2 = 2, X_SEL = 4, X_SLD = 8, X_ALL = 16;
template <int X, int R>
__global__ __launch_bounds__(64, 2) void kx(const double* in, double* out, int iters, const Rec4* __restrict__ tab,
                                            int ev, int lim, int nlo, int nhi) {
  __shared__ double ring[4][544];
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  for (int q = l; q < 544; q += 16) ring[row][q] = in[(q + row) & 255] + 1e-3 * q;
  __syncthreads();
  double acc[A], Xb[A], Yb[A];
  for (int u = 0; u < A; ++u) { acc[u] = 0; Xb[u] = in[u + l]; Yb[u] = in[u + 20 + l]; }
  double cur = ring[row][l];
  constexpr bool br1 = (X & (X_BR1 | X_ALL)) != 0, br2 = (X & (X_BR2 | X_ALL)) != 0, sel = (X & (X_SEL | X_ALL)) != 0;
  constexpr bool takein = (X & (X_SLD | X_ALL)) != 0 || R > 0;
  int k = 0;
  Rec4 nx = tab[0];
  auto request = [&]() { ++k; nx = tab[__builtin_amdgcn_readfirstlane(k & 63)]; };
  auto checks = [&](int n) {
    if constexpr (br1) {
      if (n >= ev) {  // never
        out[blockIdx.x * 64 + threadIdx.x] = acc[0];
        ev = nx.x;
        request();
      }
    }
    if constexpr (br2) {
      if (n >= lim) {  // never
        lim += 256;
        ring[row][(n + l) & 511] = in[n & 4095];
      }
    }
  };
  // FULL: the block with its extras; otherwise the bare ldsrev block
  auto blk = [&](auto full, int n, double (&lo)[A], const double (&hi)[A]) {
    constexpr bool FULL = decltype(full)::value;
    const int n0 = n & 511;
    if constexpr (FULL) checks(n);
    if constexpr (FULL && takein) asm volatile("" ::"s"(nx));
    const int base = (n0 + A * l) & 510;
#pragma unroll
    for (int q = 0; q < A; ++q) lo[q] = ring[row][base + q];
    double c = cur;
    cur = ring[row][(n0 + A + l) & 511];
    if constexpr (FULL && (X & X_SLD) != 0) request();
    if constexpr (FULL && sel) {
      const int pos = n + l, hi_m = min(n + A, nhi), lo_m = max(max(ev, n), nlo);
      c = (pos >= lo_m && pos < hi_m) ? c : 0.0;
    }
    double cm;
    asm volatile("v_mov_b64 %0, %1\n\ts_nop 1" : "=v"(cm) : "v"(c));
    fma_seq<1, true>(acc, cm, lo, hi);
  };
  if constexpr (R == 0) {
    for (int it = 0; it < iters; ++it) {
      blk(std::true_type{}, it * 2 * A, Xb, Yb);
      blk(std::true_type{}, it * 2 * A + A, Yb, Xb);
    }
  } else {
    for (int it = 0; it < iters;) {
      checks(it * 2 * A);
      asm volatile("" ::"s"(nx));
      const int run = nx.y;  // = R
      request();
#pragma unroll 1
      for (int e = it + run; it < e; ++it) {
        blk(std::false_type{}, it * 2 * A, Xb, Yb);
        blk(std::false_type{}, it * 2 * A + A, Yb, Xb);
      }
    }
  }
  double s = 0;
  for (int u = 0; u < A; ++u) s += acc[u];
  out[blockIdx.x * 64 + threadIdx.x] = s;
}

template <int X, int R>
static void runx(const char* name, const double* in, double* out, Rec4* tab, int waves, int iters) {
  int h[64][4];
  for (auto& r : h) { r[0] = INT_MAX; r[1] = R; r[2] = r[3] = 0; }
  hipMemcpy(tab, h, sizeof(h), hipMemcpyHostToDevice);
  hipEvent_t a, b;
  hipEventCreate(&a); hipEventCreate(&b);
  auto go = [&](int n) {
    hipLaunchKernelGGL((kx<X, R>), dim3(waves), dim3(64), 0, 0, in, out, n, tab, INT_MAX, INT_MAX, INT_MIN, INT_MAX);
  };
  go(16);
  hipEventRecord(a);
  go(iters);
  hipEventRecord(b);
  hipEventSynchronize(b);
  float ms = 0;
  hipEventElapsedTime(&ms, a, b);
  const double flops = 2.0 * 2 * A * A * 64.0 * waves * (double)iters;
  printf("%-8s waves %5d  %.3f ms  %.1f TFLOP/s\n", name, waves, ms, flops / ms / 1e9);
}

template <int MODE>
static void launch(dim3 g, const double* in, double* out, int iters) {
  if constexpr (MODE == 5) hipLaunchKernelGGL((krev<0, false, false>), g, dim3(64), 0, 0, in, out, iters);
  else if constexpr (MODE == 6) hipLaunchKernelGGL((krev<1, true, true>), g, dim3(64), 0, 0, in, out, iters);
  else if constexpr (MODE == 7) hipLaunchKernelGGL((krev<1, false, true>), g, dim3(64), 0, 0, in, out, iters);
  else if constexpr (MODE == 8) hipLaunchKernelGGL((krev<1, true, false>), g, dim3(64), 0, 0, in, out, iters);
  else if constexpr (MODE == 9) hipLaunchKernelGGL(k22, g, dim3(64), 0, 0, in, out, iters);
  else if constexpr (MODE == 4) hipLaunchKernelGGL(kdw, g, dim3(64), 0, 0, in, out, iters);
  else if constexpr (MODE == 3) hipLaunchKernelGGL(kpf, g, dim3(64), 0, 0, in, out, iters);
  else hipLaunchKernelGGL(k<MODE>, g, dim3(64), 0, 0, in, out, iters);
}
template <int MODE>
static void run(const char* name, const double* in, double* out, int waves, int iters, bool blocks_too = false) {
  hipEvent_t a, b;
  hipEventCreate(&a); hipEventCreate(&b);
  launch<MODE>(dim3(waves), in, out, 10);
  hipEventRecord(a);
  launch<MODE>(dim3(waves), in, out, iters);
  hipEventRecord(b);
  hipEventSynchronize(b);
  float ms = 0;
  hipEventElapsedTime(&ms, a, b);
  const double flops = (MODE == 3 ? 1.0 : 2.0) * 2 * A * A * 64.0 * waves * (double)iters;  // kpf: one block per it
  if (MODE == 9 || blocks_too)  // fc mode: blocks of A positions per second (all waves), and 200 FLOP per block and lane
    printf("%-8s waves %5d  %.3f ms  %.3e blocks/s  %.1f effective TFLOP/s\n", name, waves, ms,
           2.0 * waves * (double)iters / ms * 1e3, flops / ms / 1e9);
  else
    printf("%-8s waves %5d  %.3f ms  %.1f TFLOP/s\n", name, waves, ms, flops / ms / 1e9);
}

// vsweep_mix       : the instruction mixes
// vsweep_mix ctl   : ldsrev against the kx modes (the kernel's per-block control flow), twice over so that
//                    the run-to-run spread stands next to the differences
// vsweep_mix fc    : ldsrev against fc22 (the 2x2 fast-correlation block), alternating, six times over
int main(int argc, char** argv) {
  double *in, *out;
  hipMalloc(&in, 4096 * sizeof(double));
  hipMalloc(&out, 65536 * 64 * sizeof(double));
  double h[4096];
  for (int i = 0; i < 4096; ++i) h[i] = 1.0 + 1e-6 * i;
  hipMemcpy(in, h, sizeof(h), hipMemcpyHostToDevice);
  if (argc > 1 && !strcmp(argv[1], "fc")) {
    for (int rep = 0; rep < 6; ++rep) {
      run<6>("ldsrev", in, out, 2048, 20000, true);
      run<9>("fc22", in, out, 2048, 20000);
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "ctl")) {
    Rec4* tab;
    hipMalloc(&tab, 64 * sizeof(Rec4));
    for (int rep = 0; rep < 2; ++rep)
      for (int waves : {1024, 2048}) {
        run<6>("ldsrev", in, out, waves, 20000);
        runx<0, 0>("kx", in, out, tab, waves, 20000);
        runx<X_BR1, 0>("br1", in, out, tab, waves, 20000);
        runx<X_BR1 | X_BR2, 0>("br2", in, out, tab, waves, 20000);
        runx<X_SEL, 0>("sel", in, out, tab, waves, 20000);
        runx<X_SLD, 0>("sld", in, out, tab, waves, 20000);
        runx<X_ALL, 0>("all", in, out, tab, waves, 20000);
        runx<X_ALL, 1>("run1", in, out, tab, waves, 20000);
        runx<X_ALL, 2>("run2", in, out, tab, waves, 20000);
        runx<X_ALL, 4>("run4", in, out, tab, waves, 20000);
        runx<X_ALL, 8>("run8", in, out, tab, waves, 20000);
        runx<X_ALL, 16>("run16", in, out, tab, waves, 20000);
      }
    return 0;
  }
  for (int waves : {1024, 2048, 4096, 8192}) {
    run<0>("fma", in, out, waves, 20000);
    run<1>("dpp", in, out, waves, 20000);
    run<2>("lds", in, out, waves, 20000);
    run<3>("ldspf", in, out, waves, 40002);
    run<4>("dppwin", in, out, waves, 20000);
    run<5>("ldsdpp", in, out, waves, 20000);
    run<6>("ldsrev", in, out, waves, 20000);
    run<7>("ldsrev0", in, out, waves, 20000);
    run<8>("ldsrevc", in, out, waves, 20000);
  }
  return 0;
}
