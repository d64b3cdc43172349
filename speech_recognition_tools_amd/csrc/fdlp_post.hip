// fdlp_post.hip -- gfx950 kernel of the feature post-processing chain every consumer of the reference runs on
// the arks (decode.sh:84-90, get_Tandem_feats.sh:31-35, src/nnet/data_prep_*.py):
//   apply-cmvn   y = fl32(fl32(x * scale[d]) + offset[d])      (two roundings; the multiply only with --norm-vars)
//   add-deltas   block i of frame t = sum_j scales[i][j] * y[clamp(t + j, 0, T-1)]   (float32, ascending j)
//   splice-feats row t = [z[clamp(t-L)] .. z[clamp(t+R)]] of the delta-augmented rows z
// in one launch over a batch of concatenated utterances: every input row is read once per tile it touches,
// every output row is written once, and nothing in between goes through HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdlp_device.h"

namespace fdlp {

// A workgroup owns PostTile: tf consecutive frames t0 .. of one utterance.  LDS:
//   A [tf + L + R + 2H][D]   (only with deltas, H = order * window) the CMVN'd input frames lo .. hi-1,
//                            lo = max(0, t0 - L - H), hi = min(T, t0 + tf + R + H)
//   B [tf + L + R][D']       the delta-augmented rows of the unclamped frames u = t0 - L .. t0 + tf + R - 1
//                            (a row holds the values of frame clamp(u, 0, T-1)), D' = D (order + 1)
// Output row t0 + r is then the contiguous slice B[r D' .. r D' + (L + R + 1) D'), and the tile's output is one
// contiguous global range, streamed out with 16-byte stores between a scalar head and tail.
constexpr int kPostThreads = 256;
constexpr int kPostLdsMax = 160 * 1024;
constexpr int kPostLdsTarget = 64 * 1024;  // two workgroups per CU: one loads while the other stores
constexpr size_t kPostLdsNoAttr = 64 * 1024;  // dynamic LDS a launch may ask for without raising the kernel's limit
constexpr int kPostTileMax = 128;
constexpr int kXfKC = 32;         // columns k of the transform staged in LDS at a time
constexpr int kXfColBlocks = 4;   // 16-column blocks of the result a wave accumulates at once
// Stage ablation for benchmarks/post_throughput.py (a variant library built with -DFDLP_POST_SKIP=n, never the
// default build): bit 0 skips the global loads (frames of zeros), bit 1 the delta filter, bit 2 the stores.
#ifndef FDLP_POST_SKIP
#define FDLP_POST_SKIP 0
#endif

static inline size_t post_a_floats(int tf, int D, int order, int window, int L, int R) {
  if (order == 0) return 0;
  const size_t a = ((size_t)tf + L + R + 2 * (size_t)order * window) * D;
  return (a + 3) / 4 * 4;  // B starts 16-byte aligned
}

size_t post_lds_bytes(int tf, int D, int order, int window, int L, int R) {
  return sizeof(float) * (post_a_floats(tf, D, order, window, L, R) + ((size_t)tf + L + R) * D * (order + 1));
}

// extra: LDS bytes the workgroup needs beside the two tiles (the transform's matrix chunk)
int post_pick_tile(int D, int order, int window, int L, int R, size_t extra) {
  for (int tf = kPostTileMax; tf >= 1; tf >>= 1)
    if (post_lds_bytes(tf, D, order, window, L, R) + extra <= (size_t)kPostLdsTarget) return tf;
  return post_lds_bytes(1, D, order, window, L, R) + extra <= (size_t)kPostLdsMax ? 1 : 0;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the two roundings of ApplyCmvn stay separate (no contraction into an FMA)
__device__ __forceinline__ float cmvn1(float v, float s, float o, bool mul) {
  if (mul) v = __fmul_rn(v, s);
  return __fadd_rn(v, o);
}

// MODE -1: no deltas; 0: any order and window (taps read from the table as they are used); 1 .. kPostSpecMax:
// delta order MODE with window 2 (Kaldi's default), the taps in registers and the frame's 4 MODE + 1 input rows
// read from LDS once.  All modes perform the same float32 operations in the same order.
constexpr int kPostSpecMax = 2;  // order 3 would keep 27 taps in SGPRs and spill four of them
constexpr int kPostSpecWindow = 2;

// (r, q) = (e / n, e % n) of a thread's first element and the carry-stepping to its next one, kPostThreads on
struct DivStep {
  int r, q, dr, dq, n;
  __device__ __forceinline__ DivStep(int e, int n_) : n(n_) {
    r = e / n;
    q = e - r * n;
    dr = kPostThreads / n;
    dq = kPostThreads - dr * n;
  }
  __device__ __forceinline__ void next() {
    r += dr;
    q += dq;
    if (q >= n) {
      q -= n;
      ++r;
    }
  }
};

// -----------------------------------------------------------------------------------------------------------
// transform-feats as the last stage: out[r][n] = sum_k A[r][k] M[n][k] (+ M[n][K]) with the tile's spliced rows
// A[r][k] = B[r D' + k] (an implicit im2col: nothing is copied) on v_mfma_f32_16x16x4_f32, which is exact float32:
// each result is one fmaf chain acc = fma(A[r][k], M[n][k], acc) from acc = 0, one rounding per k, then one float32
// add of the offset column.  The chain visits k in the order
//     for g = 0, 16, 32, ..:  for s = 0 .. 3:  for q = 0 .. 3:  k = g + 4 q + s     (k >= K skipped)
// (MFMA step s of group g takes its four k from the four lane groups q, and a lane group owns four CONSECUTIVE k
// of a group: with D' a multiple of 4 a lane reads them with one 16-byte LDS load, where k = g + 4 s + q would
// cost four 4-byte loads whose 16 rows, D' floats apart, collide on the 32 banks of ds_read_b32.)  The order is a
// function of K alone: not of the tile, of D', of the k-chunks the matrix is staged in, nor of the batch.
//   * a wave owns the 16-row blocks wave and wave + 4 of the tile and all NCB column blocks of the current group,
//     so an A operand read from LDS feeds NCB MFMAs and a B operand two;
//   * the matrix M[n_mat][N][C] is read from global memory in chunks of kXfKC columns k, stored to LDS as
//     Ms[k][S] (S = 4 mod 8 floats: the k rows 4 q + s of the lane groups q fall into disjoint banks), zero where
//     k >= K or n >= N, in two buffers: the next chunk's loads are in flight while the current one is
//     multiplied, and one barrier per chunk separates a buffer's writers from its readers;
//   * A[r][k >= K] is the next row's data or whatever lies past B, so it is SELECTED to zero, never multiplied
//     by a zero; rows past tf read row tf - 1 (inside B) and are not stored.
// -----------------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

static inline int xform_ncb(int N) { return min((N + 15) / 16, kXfColBlocks); }
static inline int xform_ms_stride(int ncb) { return ncb * 16 + 4; }
// two chunks: one is multiplied while the next is written, with one barrier per chunk
size_t xform_ms_bytes(int N) { return sizeof(float) * 2 * (size_t)kXfKC * xform_ms_stride(xform_ncb(N)); }

// The MFMAs of one staged chunk for a wave's row blocks (TWO: both of them).  mlane: the chunk at row 4 q, column li;
// k0: the chunk's first k, kq: k0 + 4 q.  FULL: the whole chunk lies below K (no selects), VEC: 16-byte loads of A (D' a multiple of 4).
template <int NCB, int S, bool TWO, bool FULL, bool VEC>
__device__ __forceinline__ void xform_chunk(f32x4 (&acc0)[NCB], f32x4 (&acc1)[NCB], const float* __restrict__ B,
                                            const float* __restrict__ mlane, int a0, int a1, int k0, int kq,
                                            int K, int blds) {
  (void)blds;
  static_assert(FULL || !VEC, "the tail reads element by element");
#pragma unroll
  for (int g = 0; g < kXfKC / 16; ++g) {
    const int kg = kq + 16 * g;  // this lane's k of step s is kg + s
    if (!FULL && k0 + 16 * g >= K) break;  // the group starts at or past K
    f32x4 x0, x1 = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (VEC) {
      FDLP_CHECK(kg + 3 < K && a0 + kg + 3 < blds && a1 + kg + 3 < blds && ((a0 + kg) & 3) == 0 && ((a1 + kg) & 3) == 0);
      x0 = *(const f32x4*)(B + a0 + kg);
      if (TWO) x1 = *(const f32x4*)(B + a1 + kg);
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = kg + s, kc = FULL ? k : min(k, K - 1);
        FDLP_CHECK(kc >= 0 && kc < K && a0 + kc < blds && a1 + kc < blds);
        x0[s] = B[a0 + kc];
        if (TWO) x1[s] = B[a1 + kc];
        if (!FULL) {
          x0[s] = k < K ? x0[s] : 0.f;
          x1[s] = k < K ? x1[s] : 0.f;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (!FULL && k0 + 16 * g + s >= K) break;  // no lane group has a k < K in this step
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const float bv = mlane[(16 * g + s) * S + cb * 16];
        acc0[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[s], bv, acc0[cb], 0, 0, 0);
        if (TWO) acc1[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[s], bv, acc1[cb], 0, 0, 0);
      }
    }
  }
}

template <int NCB>
__device__ __forceinline__ void xform_stage(const PostConsts& c, const XformConsts& xc, const PostTile& tl, int tf,
                                            int nb, const float* __restrict__ B, float* __restrict__ Ms,
                                            const float* __restrict__ mats, float* __restrict__ out) {
  constexpr int S = NCB * 16 + 4;
  constexpr int NPRE = 2 * NCB;  // NCB 16 kXfKC elements of a chunk over kPostThreads threads
  static_assert(kXfKC == 32 && kPostThreads == 256, "the chunk's element map below");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // in an SGPR: the branches on it are scalar
  const int K = c.Dout, Dp = c.Dp, N = xc.N, C = xc.C;
  const int blds = nb * Dp;
  const float* __restrict__ Mg = mats + (size_t)tl.mat * N * C;
  float* o = out + (tl.row0 + tl.t0) * (int64_t)N;
  const int li = lane & 15, lq = lane >> 4;
  const int nrb = (tf + 15) >> 4;
  const bool act0 = wave < nrb, act1 = wave + 4 < nrb;
  const int a0 = min(wave * 16 + li, tf - 1) * Dp, a1 = min((wave + 4) * 16 + li, tf - 1) * Dp;
  // chunk element i of this thread: column block i / 2, k row 4 wave + lq + 16 (i % 2), column li of the block
  const int ekq = 4 * wave + lq;
  const bool vec = (Dp & 3) == 0;  // B is 16-byte aligned (post_a_floats), so every row of it is
  FDLP_CHECK(xc.ms_off >= c.a_floats + (c.tf + c.L + c.R) * Dp && tl.mat >= 0 && tl.mat < xc.n_mat);

  for (int n0 = 0; n0 < N; n0 += NCB * 16) {
    f32x4 acc0[NCB], acc1[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc0[cb] = acc1[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float pre[NPRE];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int i = 0; i < NPRE; ++i) {
        const int n = n0 + (i >> 1) * 16 + li, k = k0 + ekq + 16 * (i & 1);
        float v = 0.f;
        if (n < N && k < K) {
          FDLP_CHECK((int64_t)n * C + k < (int64_t)N * C);
          v = Mg[(size_t)n * C + k];
        }
        pre[i] = v;
      }
    };
    fetch(0);
    __syncthreads();  // the previous group's last chunk has been read
    int buf = 0;
    for (int k0 = 0; k0 < K; k0 += kXfKC, buf ^= 1) {
      float* Mc = Ms + buf * (kXfKC * S);  // read two barriers ago
#pragma unroll
      for (int i = 0; i < NPRE; ++i) {
        const int at = (ekq + 16 * (i & 1)) * S + (i >> 1) * 16 + li;
        FDLP_CHECK(at >= 0 && at < kXfKC * S);
        Mc[at] = pre[i];
      }
      __syncthreads();
      if (k0 + kXfKC < K) fetch(k0 + kXfKC);
      if (!act0) continue;
      const float* mlane = Mc + 4 * lq * S + li;
      const int kq = k0 + 4 * lq;
      if (k0 + kXfKC <= K) {
        if (vec) {
          if (act1) xform_chunk<NCB, S, true, true, true>(acc0, acc1, B, mlane, a0, a1, k0, kq, K, blds);
          else xform_chunk<NCB, S, false, true, true>(acc0, acc1, B, mlane, a0, a1, k0, kq, K, blds);
        } else {
          if (act1) xform_chunk<NCB, S, true, true, false>(acc0, acc1, B, mlane, a0, a1, k0, kq, K, blds);
          else xform_chunk<NCB, S, false, true, false>(acc0, acc1, B, mlane, a0, a1, k0, kq, K, blds);
        }
      } else {
        if (act1) xform_chunk<NCB, S, true, false, false>(acc0, acc1, B, mlane, a0, a1, k0, kq, K, blds);
        else xform_chunk<NCB, S, false, false, false>(acc0, acc1, B, mlane, a0, a1, k0, kq, K, blds);
      }
    }
    // results: lane holds column li of rows 4 lq .. 4 lq + 3 of each 16 x 16 block
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int n = n0 + cb * 16 + li;
      if (n >= N) continue;
      const float off = xc.affine ? Mg[(size_t)n * C + K] : 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (!(h ? act1 : act0)) continue;
        const f32x4 a = h ? acc1[cb] : acc0[cb];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = (wave + 4 * h) * 16 + 4 * lq + q;
          if (r >= tf) continue;
          FDLP_CHECK(r >= 0 && tl.t0 + r < tl.T && n < N);
          o[(int64_t)r * N + n] = xc.affine ? __fadd_rn(a[q], off) : a[q];
        }
      }
    }
  }
}

// NCB = 0: the rows are streamed out (post_kernel); NCB = 1 .. kXfColBlocks: they are multiplied by the transform
// instead, NCB 16-column blocks of the result at a time (xform_kernel, xform_stage above).
template <int MODE, int NCB>
__device__ __forceinline__ void post_body(const PostConsts& c, const PostTile* __restrict__ tiles,
                                          const float* __restrict__ x, int64_t n_rows,
                                          const float* __restrict__ norm, int norm_mul, float* __restrict__ out,
                                          const XformConsts& xc, const float* __restrict__ mats) {
  extern __shared__ float4 post_sh4[];
  float* sh = (float*)post_sh4;
  const PostTile tl = tiles[blockIdx.x];
  const int tid = threadIdx.x;
  const int T = tl.T, t0 = tl.t0, D = c.D, L = c.L, R = c.R;
  const int tf = min(c.tf, T - t0);
  constexpr bool DELTA = MODE >= 0;
  const int H = DELTA ? c.order * c.window : 0;
  const int lo = max(0, t0 - L - H), hi = min(T, t0 + tf + R + H);
  const int nb = tf + L + R;  // rows of B in use
  float* A = sh;
  float* B = sh + c.a_floats;
  FDLP_CHECK(tf >= 1 && t0 >= 0 && lo < hi && tl.row0 >= 0 && tl.row0 + T <= n_rows);
  FDLP_CHECK(hi - lo <= c.tf + L + R + 2 * H);

  // 1. frames lo .. hi-1 -> LDS, CMVN on the way.  Without deltas they go straight to their rows of B.
  float* dst = DELTA ? A : B + (lo - (t0 - L)) * D;
  const float* sc = norm ? norm + (size_t)tl.norm * 2 * c.Din : nullptr;
  const float* of = norm ? sc + c.Din : nullptr;
  const float* src = x + (tl.row0 + lo) * c.Din;
  const bool mul = norm_mul != 0;
  if (c.vec4) {
    const int D4 = D >> 2;
    const int n4 = (hi - lo) * D4;
    DivStep ds(tid, D4);
    for (int e = tid; e < n4; e += kPostThreads, ds.next()) {
      const int r = ds.r, q = ds.q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!(FDLP_POST_SKIP & 1)) v = ((const float4*)(src + (int64_t)r * c.Din))[q];
      if (norm) {
        const float4 s4 = ((const float4*)sc)[q], o4 = ((const float4*)of)[q];
        v.x = cmvn1(v.x, s4.x, o4.x, mul);
        v.y = cmvn1(v.y, s4.y, o4.y, mul);
        v.z = cmvn1(v.z, s4.z, o4.z, mul);
        v.w = cmvn1(v.w, s4.w, o4.w, mul);
      }
      ((float4*)(dst + r * D))[q] = v;
    }
  } else {
    const int n1 = (hi - lo) * D;
    DivStep ds(tid, D);
    for (int e = tid; e < n1; e += kPostThreads, ds.next()) {
      const int r = ds.r, d = ds.q;
      float v = 0.f;
      if (!(FDLP_POST_SKIP & 1)) v = src[(int64_t)r * c.Din + d];
      if (norm) v = cmvn1(v, sc[d], of[d], mul);
      dst[e] = v;
    }
  }
  __syncthreads();

  if constexpr (MODE > 0) {
    // 2. delta-augmented rows of the unclamped frames u = t0 - L + m: the filter runs on the edge-clamped
    //    input (DeltaFeatures::Process), block 0 is the frame itself, zero taps are skipped as Kaldi does
    constexpr int W = kPostSpecWindow, HW = MODE * W, NT = MODE + W * MODE * (MODE + 1);
    float taps[NT];  // scales[1] .. scales[MODE], uniform
#pragma unroll
    for (int k = 0; k < NT; ++k) taps[k] = c.scales[1 + k];
    const int n2 = nb * D;
    DivStep ds(tid, D);
    for (int e = tid; e < n2; e += kPostThreads, ds.next()) {
      const int m = ds.r, d = ds.q;
      const int cc = clampi(t0 - L + m, 0, T - 1);
      float w[2 * HW + 1];
#pragma unroll
      for (int j = -HW; j <= HW; ++j) {
        const int f = clampi(cc + j, 0, T - 1);
        FDLP_CHECK(f >= lo && f < hi);
        w[j + HW] = A[(f - lo) * D + d];
      }
      float* brow = B + m * c.Dp + d;
      brow[0] = w[HW];
      int tp = 0;
#pragma unroll
      for (int i = 1; i <= MODE; ++i) {
        const int hw = i * W;
        float acc = 0.f;
        if (!(FDLP_POST_SKIP & 2)) {
#pragma unroll
          for (int j = -hw; j <= hw; ++j) {
            const float sj = taps[tp + j + hw];
            if (sj != 0.f) acc = __fmaf_rn(sj, w[HW + j], acc);
          }
        }
        tp += 2 * hw + 1;
        brow[i * D] = acc;
      }
    }
  } else if constexpr (MODE == 0) {
    const int n2 = nb * D;
    DivStep ds(tid, D);
    for (int e = tid; e < n2; e += kPostThreads, ds.next()) {
      const int m = ds.r, d = ds.q;
      const int cc = clampi(t0 - L + m, 0, T - 1);
      float* brow = B + m * c.Dp + d;
      FDLP_CHECK(cc >= lo && cc < hi);
      brow[0] = A[(cc - lo) * D + d];
      for (int i = 1; i <= c.order; ++i) {
        const int hw = i * c.window;
        const float* s = c.scales + c.soff[i] + hw;
        float acc = 0.f;
        if (!(FDLP_POST_SKIP & 2)) {
          for (int j = -hw; j <= hw; ++j) {
            const float sj = s[j];
            const int f = clampi(cc + j, 0, T - 1);
            FDLP_CHECK(f >= lo && f < hi);
            if (sj != 0.f) acc = __fmaf_rn(sj, A[(f - lo) * D + d], acc);
          }
        }
        brow[i * D] = acc;
      }
    }
  } else {
    // 2'. no deltas: only the replicated edge rows of B are missing (u < 0 or u >= T)
    const int n2 = L + R > 0 ? nb * D : 0;
    DivStep ds(tid, D);
    for (int e = tid; e < n2; e += kPostThreads, ds.next()) {
      const int m = ds.r, d = ds.q;
      const int u = t0 - L + m;
      if (u < lo || u >= hi) {
        const int cc = clampi(u, 0, T - 1);
        FDLP_CHECK(cc >= lo && cc < hi && (u < 0 || u >= T));
        B[e] = B[(cc - (t0 - L)) * D + d];
      }
    }
    FDLP_CHECK(L + R > 0 || (lo == t0 && hi == t0 + tf));
  }
  __syncthreads();

  if constexpr (NCB > 0) {
    xform_stage<NCB>(c, xc, tl, tf, nb, B, sh + xc.ms_off, mats, out);
    return;
  }
  // 3. the tile's output range [(row0 + t0) Dout, (row0 + t0 + tf) Dout): element g is row r = g / Dout,
  //    column k = g % Dout, and lives at B[r D' + k]
  if (FDLP_POST_SKIP & 4) return;
  const int Dout = c.Dout, Dp = c.Dp;
  float* o = out + (tl.row0 + t0) * (int64_t)Dout;
  const int n = tf * Dout;
  const int blds = nb * Dp;
  (void)blds;  // read by the range checks only
  int head = 0, nvec = 0;
  if (Dout >= 4) {  // k + 3 wraps into the next row at most once
    head = min(n, (int)(((16u - (unsigned)((uintptr_t)o & 15u)) & 15u) >> 2));
    nvec = (n - head) >> 2;
  }
  if (nvec > 0) {
    const int wrap = Dout - Dp;  // a column past Dout is column k - Dout of the next row: LDS index - (L + R) D'
    int g = head + 4 * tid;
    int r = g / Dout, k = g - r * Dout;
    for (int v = tid; v < nvec; v += kPostThreads) {
      const int li = r * Dp + k;
      const int i0 = li, i1 = li + 1 - (k + 1 >= Dout ? wrap : 0), i2 = li + 2 - (k + 2 >= Dout ? wrap : 0),
                i3 = li + 3 - (k + 3 >= Dout ? wrap : 0);
      FDLP_CHECK(i0 >= 0 && i0 < blds && i1 >= 0 && i1 < blds && i2 >= 0 && i2 < blds && i3 >= 0 && i3 < blds);
      FDLP_CHECK(head + 4 * v + 3 < n && (((uintptr_t)(o + head + 4 * v)) & 15u) == 0);
      *(float4*)(o + head + 4 * v) = make_float4(B[i0], B[i1], B[i2], B[i3]);
      k += c.kstep;
      r += c.rstep;
      if (k >= Dout) {
        k -= Dout;
        ++r;
      }
    }
  }
  // scalar head and tail (everything when Dout < 4)
  const int ntail = n - head - 4 * nvec;
  for (int e = tid; e < head + ntail; e += kPostThreads) {
    const int g = e < head ? e : e + 4 * nvec;
    const int r = g / Dout, k = g - r * Dout;
    FDLP_CHECK(g >= 0 && g < n && r * Dp + k < blds);
    o[g] = B[r * Dp + k];
  }
}

template <int MODE>
__global__ __launch_bounds__(kPostThreads) void post_kernel(PostConsts c, const PostTile* __restrict__ tiles,
                                                            const float* __restrict__ x, int64_t n_rows,
                                                            const float* __restrict__ norm, int norm_mul,
                                                            float* __restrict__ out) {
  post_body<MODE, 0>(c, tiles, x, n_rows, norm, norm_mul, out, XformConsts{}, nullptr);
}

template <int MODE, int NCB>
__global__ __launch_bounds__(kPostThreads) void xform_kernel(PostConsts c, XformConsts xc,
                                                             const PostTile* __restrict__ tiles,
                                                             const float* __restrict__ x, int64_t n_rows,
                                                             const float* __restrict__ norm, int norm_mul,
                                                             const float* __restrict__ mats,
                                                             float* __restrict__ out) {
  post_body<MODE, NCB>(c, tiles, x, n_rows, norm, norm_mul, out, xc, mats);
}

// the delta stage's code object: post_kernel<MODE> and xform_kernel<MODE, NCB> are picked by this and nothing else
int post_mode(int order, int window) {
  return order == 0 ? -1 : (window == kPostSpecWindow && order <= kPostSpecMax ? order : 0);
}

hipError_t launch_post(const PostConsts& c, const PostTile* tiles, int ntiles, const float* x, int64_t n_rows,
                       const float* norm, int norm_mul, float* out, hipStream_t s) {
  if (ntiles <= 0) return hipSuccess;
  const size_t lds = post_lds_bytes(c.tf, c.D, c.order, c.window, c.L, c.R);
#define FDLP_POST_LAUNCH(M)                                                                                       \
  do {                                                                                                            \
    if (lds > kPostLdsNoAttr) {                                                                                   \
      const hipError_t e = hipFuncSetAttribute((const void*)post_kernel<M>,                                       \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);             \
      if (e != hipSuccess) return e;                                                                              \
    }                                                                                                             \
    hipLaunchKernelGGL(post_kernel<M>, dim3(ntiles), dim3(kPostThreads), lds, s, c, tiles, x, n_rows, norm,       \
                       norm_mul, out);                                                                            \
  } while (0)
  switch (post_mode(c.order, c.window)) {
    case -1: FDLP_POST_LAUNCH(-1); break;
    case 1: FDLP_POST_LAUNCH(1); break;
    case 2: FDLP_POST_LAUNCH(2); break;
    default: FDLP_POST_LAUNCH(0); break;
  }
#undef FDLP_POST_LAUNCH
  return hipGetLastError();
}

// What launch_xform runs for a plan: the template arguments and the branches xform_stage takes.  The launcher
// reads its template arguments, the LDS size and the attribute decision from here, and fdlp_xform_plan_dispatch
// reports the same struct, so the report cannot describe another launch than the one that runs.
XformDispatch xform_dispatch(const PostConsts& c, int N) {
  XformDispatch d;
  d.mode = post_mode(c.order, c.window);
  d.ncb = xform_ncb(N);
  d.groups = (N + 16 * d.ncb - 1) / (16 * d.ncb);
  d.tile = c.tf;
  d.vec = (c.Dp & 3) == 0;
  d.full_chunks = c.Dout / kXfKC;
  d.tail = c.Dout % kXfKC;
  d.post_lds = post_lds_bytes(c.tf, c.D, c.order, c.window, c.L, c.R);
  d.lds = d.post_lds + xform_ms_bytes(N);
  d.big_lds = d.lds > kPostLdsNoAttr;
  return d;
}

template <int NCB>
static hipError_t launch_xform_ncb(const PostConsts& c, const XformConsts& xc, const PostTile* tiles, int ntiles,
                                   const float* x, int64_t n_rows, const float* norm, int norm_mul,
                                   const float* mats, float* out, const XformDispatch& d, hipStream_t s) {
#define FDLP_XFORM_LAUNCH(M)                                                                                    \
  do {                                                                                                          \
    if (d.big_lds) {                                                                                            \
      const hipError_t e = hipFuncSetAttribute((const void*)xform_kernel<M, NCB>,                               \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)d.lds);         \
      if (e != hipSuccess) return e;                                                                            \
    }                                                                                                           \
    hipLaunchKernelGGL((xform_kernel<M, NCB>), dim3(ntiles), dim3(kPostThreads), d.lds, s, c, xc, tiles, x,     \
                       n_rows, norm, norm_mul, mats, out);                                                      \
  } while (0)
  switch (d.mode) {
    case -1: FDLP_XFORM_LAUNCH(-1); break;
    case 1: FDLP_XFORM_LAUNCH(1); break;
    case 2: FDLP_XFORM_LAUNCH(2); break;
    default: FDLP_XFORM_LAUNCH(0); break;
  }
#undef FDLP_XFORM_LAUNCH
  return hipGetLastError();
}

size_t xform_lds_bytes(int tf, int D, int order, int window, int L, int R, int N) {
  return post_lds_bytes(tf, D, order, window, L, R) + xform_ms_bytes(N);
}

hipError_t launch_xform(const PostConsts& c, XformConsts xc, const PostTile* tiles, int ntiles, const float* x,
                        int64_t n_rows, const float* norm, int norm_mul, const float* mats, float* out,
                        hipStream_t s) {
  if (ntiles <= 0) return hipSuccess;
  const XformDispatch d = xform_dispatch(c, xc.N);
  xc.ms_off = (int)(d.post_lds / sizeof(float));
  switch (d.ncb) {
    case 1: return launch_xform_ncb<1>(c, xc, tiles, ntiles, x, n_rows, norm, norm_mul, mats, out, d, s);
    case 2: return launch_xform_ncb<2>(c, xc, tiles, ntiles, x, n_rows, norm, norm_mul, mats, out, d, s);
    case 3: return launch_xform_ncb<3>(c, xc, tiles, ntiles, x, n_rows, norm, norm_mul, mats, out, d, s);
    default: return launch_xform_ncb<4>(c, xc, tiles, ntiles, x, n_rows, norm, norm_mul, mats, out, d, s);
  }
}

hipError_t checks_post(unsigned int* v, bool reset) { return fdlp_checks_local(v, reset); }

}  // namespace fdlp
