// fdlp_mfcc.hip -- gfx950 kernels of the MFCC baseline feature (src/featgen/computeMfccFeatures.py:122-131):
//   frame = reflect-padded x[k*hop + i - ext] * hamming(L)[i] / 2^15        (getFrames, features.py:118-154)
//   mag   = |scipy.fftpack.fft(frame, n)|, n = nfft/2 + 1 (any length: 513 = 27 * 19 at the defaults)
//   mel   = log10(mag @ createFbank(nfilters, nfft, srate).T)               (all n bins, the upper ones mirrored)
//   mfcc  = scipy.fftpack.dct(mel)[:, :13]                                   (type 2, unnormalised)
//   spliceFeats(mfcc, context)                                              (features.py:157-169)
// The DFT of arbitrary length runs as a dense real-input GEMM on v_mfma_f64_16x16x4f64 against a resident
// twiddle matrix TW [Kpad x 2 nbpad] (cos | -sin of 2 pi ((i k) mod n) / n, K = min(L, n) rows, bins
// 0 .. nb-1 = n/2): the input is real, so |X[n-k]| = |X[k]| and the host folds the filterbank's upper
// columns onto the lower ones (fold[m,k] = fb[m,k] + fb[m,n-k]).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fdlp_device.h"

namespace fdlp {

// A workgroup of 4 waves owns RT row tiles of 16 frames.  LDS: the windowed frames A [16 RT][sa] (re-used
// for the log-mel tile once the DFT is done) and the magnitudes [16 RT][sm].  Every wave multiplies all RT
// row tiles (one A value per tile and k-step) against its own column tiles (tile w, w+4, ..), kMfccNT at a
// time, so a twiddle read from L2 feeds RT MFMAs and is read once per workgroup.
constexpr int kMfccNT = 5;            // column tiles per pass (17 tiles at the defaults: 5, 4, 4, 4 per wave)
constexpr int kMfccLdsMax = 160 * 1024;
// Stage ablation for benchmarks/mfcc_throughput.py (a variant library built with -DFDLP_MFCC_SKIP=n, never the
// default build): bit 0 skips the gather (frames of zeros), bit 1 the MFMA k-loop.  The outputs are then wrong.
#ifndef FDLP_MFCC_SKIP
#define FDLP_MFCC_SKIP 0
#endif

// row strides (in doubles): sa = 2 mod 32 spreads the 16 frames x 4 k of an A read over the banks,
// sm odd does the same for the per-frame reads of the projection
static __host__ __device__ inline int mfcc_sa(int Kpad, int nfilters) {
  int s = Kpad > nfilters ? Kpad : nfilters;
  s += 2;
  while (s % 32 != 2) ++s;
  return s;
}
static __host__ __device__ inline int mfcc_sm(int nbpad) { return nbpad + 1; }

size_t mfcc_lds_bytes(int rt, int Kpad, int nbpad, int nfilters) {
  return sizeof(double) * 16 * (size_t)rt * ((size_t)mfcc_sa(Kpad, nfilters) + (size_t)mfcc_sm(nbpad));
}

int mfcc_row_tiles(int Kpad, int nbpad, int nfilters) {
  for (int rt = 2; rt >= 1; --rt)
    if (mfcc_lds_bytes(rt, Kpad, nbpad, nfilters) <= (size_t)kMfccLdsMax) return rt;
  return 0;
}

template <int RT>
__global__ __launch_bounds__(256) void mfcc_kernel(MfccConsts c, const MfccFrame* __restrict__ frames, int nframes,
                                                   const void* __restrict__ pcm, int pcm_kind,
                                                   const int16_t* __restrict__ noise, float* __restrict__ out,
                                                   double* __restrict__ out64, double* __restrict__ cep,
                                                   int decimals, double scale10) {
  extern __shared__ double mfcc_sh[];
  constexpr int M = 16 * RT;
  const int sa = mfcc_sa(c.Kpad, c.nfilters), sm = mfcc_sm(c.nbpad);
  double* A = mfcc_sh;                  // [M][sa]
  double* mag = mfcc_sh + (size_t)M * sa;  // [M][sm]
  const int f0 = blockIdx.x * M;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  // 1. gather, window, scale: A[row][i] = (s | s + alpha n)[reflect(k hop + i - ext)] * hamming[i] * 2^-15,
  //    zero past K = min(L, n) (fft(x, n) truncates a longer frame, pads a shorter one) and past nframes
  for (int row = wave; row < M; row += 4) {
    const int f = f0 + row;
    const bool live = f < nframes;
    MfccFrame fd{};
    if (live) fd = frames[f];
    FDLP_CHECK(f >= 0 && (!live || (fd.T >= 1 && fd.k >= 0 && fd.k < fd.F)));
    for (int i = lane; i < c.Kpad; i += 64) {
      double v = 0.0;
      if (live && i < c.K && !(FDLP_MFCC_SKIP & 1)) {
        const int64_t t = reflect_idx((int64_t)fd.k * c.hop + i - c.ext, fd.T);
        FDLP_CHECK(t >= 0 && t < fd.T);
        double sv;
        if (pcm_kind == 0) {
          sv = (double)((const int16_t*)pcm)[fd.pcm_off + t];
          if (fd.noise_off >= 0) sv = __dadd_rn(sv, __dmul_rn(fd.alpha, (double)noise[fd.noise_off + t]));
        } else {
          sv = ((const double*)pcm)[fd.pcm_off + t];
        }
        v = __dmul_rn(__dmul_rn(sv, c.window[i]), 0x1p-15);
      }
      FDLP_CHECK(i < sa && row * sa + i < M * sa);
      A[row * sa + i] = v;
    }
  }
  __syncthreads();

  // 2. Re / Im = A @ TW on the fp64 MFMA; 3. hypot into the magnitude tile
  const int i_lane = lane & 15, kk_lane = lane >> 4;
  const int nct = c.nbpad >> 4;
  const int tw_ld = 2 * c.nbpad;
  const int ksteps = (FDLP_MFCC_SKIP & 2) ? 0 : c.Kpad >> 2;
  for (int j0 = 0; wave + 4 * j0 < nct; j0 += kMfccNT) {
    dbl4 re[RT][kMfccNT], im[RT][kMfccNT];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int j = 0; j < kMfccNT; ++j) {
        re[r][j] = dbl4{0.0, 0.0, 0.0, 0.0};
        im[r][j] = dbl4{0.0, 0.0, 0.0, 0.0};
      }
    // tiles past nct alias the pass's first tile (read, never stored), so the unrolled body has no branches
    int col[kMfccNT];
#pragma unroll
    for (int j = 0; j < kMfccNT; ++j) {
      int ct = wave + 4 * (j0 + j);
      if (ct >= nct) ct = wave + 4 * j0;
      col[j] = 16 * ct + i_lane;
      FDLP_CHECK(ct >= 0 && ct < nct && c.nbpad + col[j] < tw_ld);
    }
    FDLP_CHECK(ksteps == 0 || kk_lane < c.Kpad);
    const double* tw = c.tw + (size_t)kk_lane * tw_ld;
    double bc[kMfccNT], bs[kMfccNT], nc[kMfccNT], ns[kMfccNT];
#pragma unroll
    for (int j = 0; j < kMfccNT; ++j) {
      bc[j] = tw[col[j]];
      bs[j] = tw[c.nbpad + col[j]];
    }
    double a[RT], an[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) a[r] = A[(16 * r + i_lane) * sa + kk_lane];
    for (int st = 0; st < ksteps; ++st) {
      // the next k-step's twiddles and A values are in flight while this one's MFMAs issue (the last
      // step re-reads its own)
      const int adv = st + 1 < ksteps ? 4 : 0;
      const double* twn = tw + (size_t)adv * tw_ld;
      FDLP_CHECK(4 * st + adv + kk_lane < c.Kpad && (16 * (RT - 1) + i_lane) * sa + 4 * st + adv + kk_lane < M * sa);
#pragma unroll
      for (int j = 0; j < kMfccNT; ++j) {
        nc[j] = twn[col[j]];
        ns[j] = twn[c.nbpad + col[j]];
      }
#pragma unroll
      for (int r = 0; r < RT; ++r) an[r] = A[(16 * r + i_lane) * sa + 4 * st + adv + kk_lane];
#pragma unroll
      for (int j = 0; j < kMfccNT; ++j)
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          re[r][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], bc[j], re[r][j], 0, 0, 0);
          im[r][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], bs[j], im[r][j], 0, 0, 0);
        }
#pragma unroll
      for (int j = 0; j < kMfccNT; ++j) {
        bc[j] = nc[j];
        bs[j] = ns[j];
      }
#pragma unroll
      for (int r = 0; r < RT; ++r) a[r] = an[r];
      tw = twn;
    }
    // C/D of the fp64 MFMA: column lane & 15, row (lane >> 4) + 4 reg
#pragma unroll
    for (int j = 0; j < kMfccNT; ++j) {
      const int ct = wave + 4 * (j0 + j);
      if (ct < nct) {
        const int k = 16 * ct + i_lane;
        if (k < c.nb) {
          FDLP_CHECK(k < sm && (16 * (RT - 1) + kk_lane + 12) * sm + k < M * sm);
#pragma unroll
          for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) mag[(16 * r + kk_lane + 4 * q) * sm + k] = hypot(re[r][j][q], im[r][j][q]);
        }
      }
    }
  }
  __syncthreads();

  // 4. folded filterbank over each filter's non-zero range, 5. log10 -> mel tile (over A)
  double* mel = A;  // [M][sa], nfilters <= sa
  for (int e = threadIdx.x; e < M * c.nfilters; e += 256) {
    const int row = e % M, m = e / M;
    const double* w = c.fold + (size_t)m * c.nb;
    const double* mg = mag + row * sm;
    double acc = 0.0;
    FDLP_CHECK(0 <= c.lo[m] && c.lo[m] <= c.hi[m] && c.hi[m] <= c.nb && row * sm + c.nb <= M * sm);
    for (int k = c.lo[m]; k < c.hi[m]; ++k) acc = fma(mg[k], w[k], acc);
    FDLP_CHECK(m < sa && row * sa + m < M * sa);
    mel[row * sa + m] = log10(acc);
  }
  __syncthreads();

  // 6. DCT-II (y[q] = 2 sum_m mel[m] cos(pi q (2m+1) / (2 nfilters))), first ncep; 7. store
  for (int e = threadIdx.x; e < M * c.ncep; e += 256) {
    const int row = e / c.ncep, q = e % c.ncep;
    const int f = f0 + row;
    if (f >= nframes) continue;
    const double* ml = mel + row * sa;
    FDLP_CHECK(row < M && row * sa + c.nfilters <= M * sa);
    double acc = 0.0;
    for (int m = 0; m < c.nfilters; ++m) acc = fma(ml[m], c.dct[m * c.ncep + q], acc);
    if (cep) {  // --context: the splice kernel rounds and stores
      cep[(int64_t)f * c.ncep + q] = acc;
    } else {
      const int64_t o = frames[f].out_row * c.ncep + q;
      FDLP_CHECK(o >= 0 && o < (int64_t)nframes * c.ncep);  // a batch's output rows are its frames
      if (out64) out64[o] = acc;
      if (out) out[o] = decimals >= 0 ? (float)(nearbyint(acc * scale10) / scale10) : (float)acc;
    }
  }
}

// spliceFeats (features.py:157-169): row k of an utterance of F frames is [mfcc[k-C] .. mfcc[k+C]] with zeros
// outside [0, F); the reference's loop stops at F - C, so rows F-C .. F-1 stay zero (every row when C >= F).
// A batch's frames are contiguous per utterance, so frame g's neighbours are cep rows g - C .. g + C.
__global__ __launch_bounds__(256) void mfcc_splice_kernel(const double* __restrict__ cep,
                                                          const MfccFrame* __restrict__ frames, int nframes, int ncep,
                                                          int C, float* __restrict__ out, double* __restrict__ out64,
                                                          int decimals, double scale10) {
  const int W = ncep * (2 * C + 1);
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)nframes * W) return;
  const int g = (int)(e / W), col = (int)(e % W);
  const MfccFrame fd = frames[g];
  double v = 0.0;
  if (fd.k < fd.F - C) {
    const int j = col / ncep, q = col % ncep;
    const int src = fd.k + j - C;
    FDLP_CHECK(!(src >= 0 && src < fd.F) || (g + j - C >= 0 && g + j - C < nframes));
    if (src >= 0 && src < fd.F) v = cep[(int64_t)(g + j - C) * ncep + q];
  }
  const int64_t o = fd.out_row * W + col;
  FDLP_CHECK(o >= 0 && o < (int64_t)nframes * W);
  if (out64) out64[o] = v;
  if (out) out[o] = decimals >= 0 ? (float)(nearbyint(v * scale10) / scale10) : (float)v;
}

hipError_t launch_mfcc(const MfccConsts& c, const MfccFrame* frames, int nframes, const void* pcm, int pcm_kind,
                       const int16_t* noise, double* cep, float* out, double* out64, int decimals, hipStream_t s) {
  if (nframes <= 0) return hipSuccess;
  double scale10 = 1.0;
  for (int i = 0; i < decimals; ++i) scale10 *= 10.0;
  const size_t lds = mfcc_lds_bytes(c.rt, c.Kpad, c.nbpad, c.nfilters);
  const int M = 16 * c.rt;
  double* scratch = c.context > 0 ? cep : nullptr;
  if (c.rt == 2) {
    if (lds > 65536)
      (void)hipFuncSetAttribute((const void*)mfcc_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(mfcc_kernel<2>, dim3((nframes + M - 1) / M), dim3(256), lds, s, c, frames, nframes, pcm,
                       pcm_kind, noise, out, out64, scratch, decimals, scale10);
  } else {
    if (lds > 65536)
      (void)hipFuncSetAttribute((const void*)mfcc_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(mfcc_kernel<1>, dim3((nframes + M - 1) / M), dim3(256), lds, s, c, frames, nframes, pcm,
                       pcm_kind, noise, out, out64, scratch, decimals, scale10);
  }
  if (c.context > 0) {
    const int64_t total = (int64_t)nframes * c.ncep * (2 * c.context + 1);
    hipLaunchKernelGGL(mfcc_splice_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cep, frames,
                       nframes, c.ncep, c.context, out, out64, decimals, scale10);
  }
  return hipGetLastError();
}

hipError_t checks_mfcc(unsigned int* v, bool reset) { return fdlp_checks_local(v, reset); }

}  // namespace fdlp
